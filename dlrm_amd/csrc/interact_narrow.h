// interact_narrow.h — the fused lookup + pairwise-dot interaction kernels for tables of D = 16 / 32 / 64, forward and backward, over a
// compile-time ROW SOURCE S (in the spirit of gather_pipeline.h's S).  interact_narrow.hip instantiates them for fp32 rows (F32Rows, below),
// interact_narrow_rows.hip for bfloat16 and 8- / 4-bit packed rows, interact_narrow_qr.hip for quotient-remainder tables.  The contract,
// the row fetch, the LDS image and the pipeline are described at the head of interact_narrow.hip; everything behind image_write —
// fragment reads, MFMA order, stores — does not know S (the backward asks S only WHERE a feature's gradient row goes).
//
// A row source supplies:
//   LB            bytes of a row that a lane loads for its 4 columns (its slot is at byte LB * lc of the row, lc = lane % (D / 4));
//   pitch(D)      bytes between two rows of a table;
//   Regs          the per-lane staged registers of one pass;
//   zero(Regs&)   the staged value of a row that is not fetched (an out-of-range id): widen() of it is four times +0.0;
//   load<D>(Regs&, slot, lc)   the loads of the lane's slot (and of what else of the row it needs), nothing waits there;
//   widen(Regs)   the four fp32 elements in front of image_write: element = fmaf(1.0f, value, +0.0f), the lookup kernels' sum of a bag of
//                 one row without per-sample weights.
// ... and, by inheriting OneArraySide (below) or by defining its own, the SELECTOR SIDE: the argument block and its LDS tables, the per-lane
// state, what the owner lane of a feature hands to the lanes of a row (Row), the row loads of a sample, the composition in front of
// image_write and the column slot of a feature's gradient row.  OneArraySide is the side of tables that are one array (fp32, bf16, packed);
// interact_narrow_qr.hip defines the side of quotient-remainder tables (two arrays, Row = (q, r), virtual gradient slots).  The members
// that need the row format take S as their first template argument.
// The rules of interact_narrow.hip hold for every source: only compiler-counted global loads / stores and LDS accesses, no inline-asm
// loads, no LDS-DMA, no hand-placed waits, optional loads as assignments under `if`, kernarg tables through LDS, scratch 0.
#pragma once
#include "gather_common.h"

namespace {

template <int D, int NB> struct NGeom {
    static constexpr int LPR = D / 4;                           // lanes per row
    static constexpr int RPP = 64 / LPR;                        // rows per pass
    static constexpr int NP = (16 * NB - 1 + RPP - 1) / RPP;    // passes: image rows 1 .. 16 NB - 1
    static constexpr int LS = D + 4;                            // image row pitch, floats
    static constexpr int IMGB = 16 * NB * LS * 4;               // bytes of an image
    static constexpr int DRB = NB == 1 ? 1024 : 3072;           // dR row image of the backward (D + P <= 200 / 592 floats); its last word stays zero
    static constexpr int NS = D / 16;                           // 16-column steps
};

// what a lane keeps across the sample loop
template <int NP>
struct NLane {
    const gchar* base[NP];      // the lane's slot of row 0 of the table behind image row 1 + RPP p + lane / LPR
    unsigned wofs[NP];          // byte offset of the lane's 16-byte slot inside the image
    bool on[NP];                // that row is a feature (< F)
    const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
    const gchar* osrc;
    long long rows;
    bool own;
};

// the selector side of one-array tables: the row number travels as one unsigned (GC_BAD: the zero row)
struct OneArraySide {
    using Args = GatherArgs;
    using Row = unsigned;
    static constexpr int NTAB = 4;              // LDS tables: [0] w  [1] idx  [2] off  [3] rows
    static constexpr bool DUP = false;          // the backward never stores a gradient row twice
    template <int NP> using Lane = NLane<NP>;
    static __device__ __forceinline__ Row none() { return GC_BAD; }

    static __device__ __forceinline__ void tables_to_lds(const Args& a, long long* tab, int F) {
        args_to_lds(a, tab, tab + GC_MAXF, tab + 2 * GC_MAXF, tab + 3 * GC_MAXF, F);
    }

    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void lane_init(NLane<NP>& nl, const long long* tab, int F, int lane) {
        using G = NGeom<D, NB>;
        const long long *tw = tab, *tq = tab + GC_MAXF, *to = tab + 2 * GC_MAXF, *tr = tab + 3 * GC_MAXF;
        const int rg = lane / G::LPR, lc = lane % G::LPR;
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            const int row = 1 + G::RPP * p + rg;
            nl.on[p] = row < F;                                   // no lane loads or writes a row for a feature slot >= F (F <= 32: inside the tables)
            nl.base[p] = nl.on[p] ? (const gchar*)tw[row] + S::LB * lc : nullptr;
            nl.wofs[p] = nl.on[p] ? (unsigned)(row * G::LS * 4 + 16 * lc) : 0u;
        }
        nl.own = lane >= 1 && lane < F;
        nl.qsrc = nl.own ? (const gchar*)tq[lane] : nullptr;
        nl.osrc = nl.own ? (const gchar*)to[lane] : nullptr;
        nl.rows = nl.own ? tr[lane] : 0;
    }

    template <typename IT, int NP>
    static __device__ __forceinline__ Row resolve(const NLane<NP>& nl, const Sel<IT>& sel, long long s, int lane, long long* err) {
        return sel_resolve<IT>(nl, sel, s, lane, err);
    }

    // row loads of one sample into registers: NP passes, the source's loads each, nothing waits here
    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void rows_issue(typename S::Regs (&v)[NP], const NLane<NP>& nl, unsigned idu, int lane) {
        using G = NGeom<D, NB>;
        const int rg = lane / G::LPR, lc = lane % G::LPR;
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            const unsigned mine = (unsigned)__shfl((int)idu, (1 + G::RPP * p + rg) & 63, 64);      // (rows that are features are < 32: a lane of this wave)
            S::zero(v[p]);
            if (nl.on[p] && mine != GC_BAD) S::template load<D>(v[p], nl.base[p] + (unsigned long long)mine * S::pitch(D), lc);      // 64-bit byte offset
        }
    }

    template <typename S, int D, int NB, int NP>
    static __device__ __forceinline__ void image_write(char* img, const typename S::Regs (&v)[NP], const NLane<NP>& nl, const float4& xv, int lane,
                                                       const Args&) {
        using G = NGeom<D, NB>;
        if (lane < G::LPR) *(float4*)(img + 16 * lane) = xv;                // row 0
#pragma unroll
        for (int p = 0; p < G::NP; ++p) {
            if (nl.on[p]) *(float4*)(img + nl.wofs[p]) = S::widen(v[p]);
        }
    }

    // the backward's row store of feature i >= 1 goes to columns slot * D .. of dE: table i - 1
    static __device__ __forceinline__ long long dst_slot(const Args&, const long long*, int i, int, bool& dup) { dup = false; return i - 1; }
};

// fp32 rows: a row of D floats is 4 D bytes, a lane's 4 columns are ONE 16-byte load
struct F32Rows : OneArraySide {
    static constexpr int LB = 16;
    static constexpr unsigned long long pitch(int D) { return 4ull * D; }
    using Regs = float4;
    static __device__ __forceinline__ void zero(Regs& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
    template <int D>
    static __device__ __forceinline__ void load(Regs& v, const gchar* slot, int) {
        const floatx4 q = *(const gfloatx4*)slot;
        v = make_float4(q.x, q.y, q.z, q.w);
    }
    static __device__ __forceinline__ float4 widen(const Regs& q) { return make_float4(bag1(q.x), bag1(q.y), bag1(q.z), bag1(q.w)); }
};

// -------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------
template <typename S, int D, int NB, typename IT>          // NB = 16-row tiles of the image: 1 (F <= 16) or 2
__global__ __launch_bounds__(256) void interact_fwd_narrow_kernel(typename S::Args na, const float* __restrict__ x, long long x_ld, long long B,
                                                                  int F, int self, float* __restrict__ R, long long ldr) {
    if (na.pred.skip()) return;                              // (the two-kernel form runs instead)
    using G = NGeom<D, NB>;
    using Regs = typename S::Regs;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = G::NP;
    constexpr int IMGB = G::IMGB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + S::NTAB * GC_MAXF) + (size_t)wave * 2 * IMGB;

    S::tables_to_lds(na, tab, F);
    for (int e = lane; e < 2 * IMGB / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);      // rows F.. (and the pitch padding) stay zero
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    typename S::template Lane<NP> nl;
    S::template lane_init<S, D, NB>(nl, tab, F, lane);

    const int P = (self & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    // where this lane's four results of tile pair (r, c) go inside the R row (float index; -1 = not part of the output):
    // output row i = 16 r + 4 g + q, column j = 16 c + li — a function of the lane only, computed once
    constexpr int NPAIR = NB * (NB + 1) / 2;
    int opos[NPAIR][4];
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 16 * r + 4 * g + q, j = 16 * c + li;
                const bool ok = i < F && ((self & 1) ? (j <= i) : (j < i));
                opos[r * (r + 1) / 2 + c][q] = ok ? D + pair_pos(i, j, F, self) : -1;
            }
    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's image, and the second sample's (checked) selectors
    typename S::Row idun;
    {
        const typename S::Row idu = S::template resolve<IT>(nl, sel_load<IT>(nl, b), b, lane, na.err);
        Regs v[NP];
        S::template rows_issue<S, D, NB>(v, nl, idu, lane);
        float4 xv = zero4;                                  // (not a ?: of two lvalues: that selects between ADDRESSES and puts zero4 into scratch)
        if (lane < G::LPR) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const long long s1 = b + b_stride;
        const Sel<IT> sel1 = sel_load<IT>(nl, s1 < B ? s1 : last);
        S::template image_write<S, D, NB>(img0, v, nl, xv, lane, na);
        idun = s1 < B ? S::template resolve<IT>(nl, sel1, s1, lane, na.err) : S::none();
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end: its image is written and never multiplied): rows out now from the selectors that were
        // loaded and checked one sample ago, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        Regs vn[NP];
        S::template rows_issue<S, D, NB>(vn, nl, idun, lane);
        float4 xn = zero4;
        if (lane < G::LPR) xn = *(const float4*)(x + (s1 < B ? s1 : last) * x_ld + 4 * lane);
        const Sel<IT> seln = sel_load<IT>(nl, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        // ---- fragments: row 16 r + li, columns 16 s + 4 g .. + 3 (interact_fwd_kernel's av / bv) ----
        float4 fr[NB][G::NS];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int s = 0; s < G::NS; ++s)
                fr[r][s] = *(const float4*)(my + ((16 * r + li) * G::LS + 16 * s + 4 * g) * 4);
        float4 xrow = zero4;
        if (lane < G::LPR) xrow = *(const float4*)(my + lane * 16);
        __builtin_amdgcn_sched_barrier(0);      // all fragment reads (and the next sample's loads) in front of the first MFMA
        floatx4 acc[NPAIR][2];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) { acc[p][0] = (floatx4){0.f, 0.f, 0.f, 0.f}; acc[p][1] = (floatx4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < G::NS; ++s) {
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

        // only now are the next sample's registers touched: the wait for its rows (and for the selectors behind them) sits here, behind
        // the multiplication and IN FRONT of this sample's stores — vmcnt counts stores too, and a wait placed behind them would wait
        // for their acknowledgement; this way they drain beside the next sample's loads and MFMAs
        S::template image_write<S, D, NB>(img0 + (cur ^ 1) * IMGB, vn, nl, xn, lane, na);
        idun = s2 < B ? S::template resolve<IT>(nl, seln, s2, lane, na.err) : S::none();

        float* Rb = R + b * ldr;
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) {
            const floatx4 sum = acc[p][0] + acc[p][1];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (opos[p][q] >= 0) Rb[opos[p][q]] = sum[q];
        }
        // R[:, 0:D] = x (row 0 of the image), then the alignment padding
        if (lane < G::LPR) *(float4*)(Rb + 4 * lane) = xrow;
        for (long long d = D + P + lane; d < ldr; d += 64) Rb[d] = 0.f;
        cur ^= 1;
    }
}

// -------------------------------------------------------------------------------------------
// backward: dT = (dZ + dZ^T) . T per sample (interact_bwd_kernel<NB>), T fetched from the tables
// -------------------------------------------------------------------------------------------
template <typename S, int D, int NB, typename IT>
__global__ __launch_bounds__(256) void interact_bwd_narrow_kernel(typename S::Args na, const float* __restrict__ x, long long x_ld, long long B,
                                                                  int F, int self, const float* __restrict__ dR, long long ldr,
                                                                  float* __restrict__ dx, long long dx_ld, float* __restrict__ dE, long long dE_ld) {
    if (na.pred.skip()) return;
    using G = NGeom<D, NB>;
    using Regs = typename S::Regs;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = G::NP;
    constexpr int IMGB = G::IMGB;
    constexpr int DRB = G::DRB;
    constexpr int NDR = DRB / 1024;
    constexpr int NS = G::NS;                 // adjacent columns of a lane: NS li .. NS li + NS - 1
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + S::NTAB * GC_MAXF) + (size_t)wave * (2 * IMGB + 2 * DRB);
    char* drow0 = img0 + 2 * IMGB;

    S::tables_to_lds(na, tab, F);
    for (int e = lane; e < (2 * IMGB + 2 * DRB) / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    typename S::template Lane<NP> nl;
    S::template lane_init<S, D, NB>(nl, tab, F, lane);
    const int P = (self & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    const int rowb = 4 * ((D + P + 3) & ~3);             // bytes of a dR row that are read (< DRB: D + P <= 200 for F <= 16, <= 592 for F <= 32)

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
                if (i == j) { if (self & 1) { off = D + pair_pos(i, i, F, self); sc = 2.f; } }
                else {
                    const int hi = i > j ? i : j, lo = i > j ? j : i;
                    off = D + pair_pos(hi, lo, F, self);
                }
            }
            a_off[r][kk] = off * 4; a_scale[r][kk] = sc;
        }
    // destination rows of this lane: i = 16 r + 4 g + q — feature 0 is dx, feature f >= 1 columns slot D .. of dE, slot = f - 1 for one-array
    // tables; a side with DUP may ask for a second copy of the row one slot further.  GLOBAL pointers.
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
            const long long slot = S::dst_slot(na, tab, i, F, dup);
            if (S::DUP && dup) dupbits |= 1u << (4 * r + q);
            const long long ld = i == 0 ? dx_ld : dE_ld;
            float* base = i == 0 ? dx : dE + slot * D;
            orow[r][q] = (i < F) ? (gchar*)(base + b * ld + NS * li) : nullptr;
            ostep[r][q] = b_stride * ld * 4;
        }

    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's images, and the second sample's (checked) selectors
    typename S::Row idun;
    {
        const typename S::Row idu = S::template resolve<IT>(nl, sel_load<IT>(nl, b), b, lane, na.err);
        Regs v[NP];
        S::template rows_issue<S, D, NB>(v, nl, idu, lane);
        float4 xv = zero4;
        if (lane < G::LPR) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const DrRegs<NDR> d = dr_load<NDR>(dR + b * ldr, rowb, lane);
        const long long s1 = b + b_stride;
        const Sel<IT> sel1 = sel_load<IT>(nl, s1 < B ? s1 : last);
        S::template image_write<S, D, NB>(img0, v, nl, xv, lane, na);
        dr_write<NDR>(drow0, d, rowb, lane);
        idun = s1 < B ? S::template resolve<IT>(nl, sel1, s1, lane, na.err) : S::none();
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end): rows, x and the dR row out now, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        const long long n1 = s1 < B ? s1 : last;
        Regs vn[NP];
        S::template rows_issue<S, D, NB>(vn, nl, idun, lane);
        float4 xn = zero4;
        if (lane < G::LPR) xn = *(const float4*)(x + n1 * x_ld + 4 * lane);
        const DrRegs<NDR> dn = dr_load<NDR>(dR + n1 * ldr, rowb, lane);
        const Sel<IT> seln = sel_load<IT>(nl, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        const char* dr = drow0 + cur * DRB;
        // A fragments: S[16 r + li][4 kk + g], rebuilt from the dR row (interact_bwd_kernel reads them from its S matrix)
        float aS[NB][4 * NB];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int kk = 0; kk < 4 * NB; ++kk) {
                const float v = *(const float*)(dr + a_off[r][kk]);
                aS[r][kk] = a_scale[r][kk] * v;
            }
        // B fragments: T[4 kk + g][NS li + c] (rows >= F of the image are zero)
        float bT[4 * NB][NS];
#pragma unroll
        for (int kk = 0; kk < 4 * NB; ++kk) {
            const float* src = (const float*)(my + ((4 * kk + g) * G::LS + NS * li) * 4);
            if constexpr (NS == 4) { const float4 t = *(const float4*)src; bT[kk][0] = t.x; bT[kk][1] = t.y; bT[kk][2] = t.z; bT[kk][3] = t.w; }
            else if constexpr (NS == 2) { const float2 t = *(const float2*)src; bT[kk][0] = t.x; bT[kk][1] = t.y; }
            else bT[kk][0] = *src;
        }
        // feature 0's two extra operands (the x part of dR; x itself for the ReLU derivative), read by every lane in front of the MFMAs
        float x0[NS], y0[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) { x0[c] = *(const float*)(dr + (NS * li + c) * 4); y0[c] = *(const float*)(my + (NS * li + c) * 4); }
        __builtin_amdgcn_sched_barrier(0);      // the next sample's loads stay in front of the multiplication
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            floatx4 acc[NS][2];
#pragma unroll
            for (int c = 0; c < NS; ++c) { acc[c][0] = (floatx4){0.f, 0.f, 0.f, 0.f}; acc[c][1] = (floatx4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int kk = 0; kk < 4 * NB; ++kk)
#pragma unroll
                for (int c = 0; c < NS; ++c)
                    acc[c][kk & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(aS[r][kk], bT[kk][c], acc[c][kk & 1], 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if ((rowbits >> (4 * r + q)) & 1u) {
                    float v[NS];
#pragma unroll
                    for (int c = 0; c < NS; ++c) {
                        v[c] = acc[c][0][q] + acc[c][1][q];
                        if (r == 0 && q == 0 && g == 0) {       // feature 0 also feeds R[:, 0:D] ...
                            v[c] += x0[c];
                            if ((self & 4) && !(y0[c] > 0.f)) v[c] = 0.f;      // ... and is a ReLU output whose derivative is applied here
                        }
                    }
                    if constexpr (NS == 4) *(gfloatx4*)orow[r][q] = (floatx4){v[0], v[1], v[2], v[3]};
                    else if constexpr (NS == 2) *(gfloatx2*)orow[r][q] = (floatx2){v[0], v[1]};
                    else *(gfloat*)orow[r][q] = v[0];
                    if constexpr (S::DUP) {
                        if ((dupbits >> (4 * r + q)) & 1u) {
                            gchar* o2 = orow[r][q] + D * 4;
                            if constexpr (NS == 4) *(gfloatx4*)o2 = (floatx4){v[0], v[1], v[2], v[3]};
                            else if constexpr (NS == 2) *(gfloatx2*)o2 = (floatx2){v[0], v[1]};
                            else *(gfloat*)o2 = v[0];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) if ((rowbits >> (4 * r + q)) & 1u) orow[r][q] += ostep[r][q];

        // only now are the next sample's registers touched (see the forward kernel)
        S::template image_write<S, D, NB>(img0 + (cur ^ 1) * IMGB, vn, nl, xn, lane, na);
        dr_write<NDR>(drow0 + (cur ^ 1) * DRB, dn, rowb, lane);
        idun = s2 < B ? S::template resolve<IT>(nl, seln, s2, lane, na.err) : S::none();
        cur ^= 1;
    }
}

template <int D, int NB>
constexpr size_t narrow_lds(bool bwd, int ntab = 4) {
    return (size_t)ntab * GC_MAXF * sizeof(long long) + (size_t)GC_WAVES * (2 * (size_t)NGeom<D, NB>::IMGB + (bwd ? 2 * (size_t)NGeom<D, NB>::DRB : 0));
}
// (The grid rule keeps the D = 64, NB = 2 backward, which needs 93 KiB, at one workgroup per CU.  Three-wave workgroups, of which two fit a CU,
// were measured SLOWER: 0.635 ms against 0.462 ms for the two-kernel form, where the four-wave launch has 0.515 against 0.464 ms —
// profiles/narrow_interact/fused_rates.md.)
template <typename S, int D, int NB, typename IT>
void launch_fwd(const typename S::Args& na, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, hipStream_t st) {
    constexpr size_t lds = narrow_lds<D, NB>(false, S::NTAB);
    dlrm_lds_limit<interact_fwd_narrow_kernel<S, D, NB, IT>>(lds);
    hipLaunchKernelGGL((interact_fwd_narrow_kernel<S, D, NB, IT>), dim3((unsigned)gather_grid(B, lds)), dim3(64 * GC_WAVES), lds, st, na, x, x_ld,
                       B, F, self, R, ldr);
}

template <typename S, int D, int NB, typename IT>
void launch_bwd(const typename S::Args& na, const float* x, long long x_ld, long long B, int F, int self, const float* dR, long long ldr, float* dx,
                long long dx_ld, float* dE, long long dE_ld, hipStream_t st) {
    constexpr size_t lds = narrow_lds<D, NB>(true, S::NTAB);
    dlrm_lds_limit<interact_bwd_narrow_kernel<S, D, NB, IT>>(lds);
    hipLaunchKernelGGL((interact_bwd_narrow_kernel<S, D, NB, IT>), dim3((unsigned)gather_grid(B, lds)), dim3(64 * GC_WAVES), lds, st, na, x, x_ld,
                       B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld);
}

// the shapes of dlrm_interact_gather_narrow_ok: D = 16 / 32 / 64, 1 <= F <= 32 (every row source takes exactly these)
static inline bool narrow_shape_ok(int F, int D) { return (D == 16 || D == 32 || D == 64) && F >= 1 && F <= GC_MAXF; }

}  // namespace

// CALL<S, D, NB, IT>(...) for the function's D, F and idx_bits; S: the row source
#define NARROW_DISPATCH(CALL, S, ...)                                                                                \
    do {                                                                                                             \
        const int key = D * 4 + (F <= 16 ? 0 : 2) + (idx_bits == 64 ? 1 : 0);                                        \
        switch (key) {                                                                                               \
            case 16 * 4 + 0: CALL<S, 16, 1, int>(__VA_ARGS__); break;  case 16 * 4 + 1: CALL<S, 16, 1, long long>(__VA_ARGS__); break;  \
            case 16 * 4 + 2: CALL<S, 16, 2, int>(__VA_ARGS__); break;  case 16 * 4 + 3: CALL<S, 16, 2, long long>(__VA_ARGS__); break;  \
            case 32 * 4 + 0: CALL<S, 32, 1, int>(__VA_ARGS__); break;  case 32 * 4 + 1: CALL<S, 32, 1, long long>(__VA_ARGS__); break;  \
            case 32 * 4 + 2: CALL<S, 32, 2, int>(__VA_ARGS__); break;  case 32 * 4 + 3: CALL<S, 32, 2, long long>(__VA_ARGS__); break;  \
            case 64 * 4 + 0: CALL<S, 64, 1, int>(__VA_ARGS__); break;  case 64 * 4 + 1: CALL<S, 64, 1, long long>(__VA_ARGS__); break;  \
            case 64 * 4 + 2: CALL<S, 64, 2, int>(__VA_ARGS__); break;  case 64 * 4 + 3: CALL<S, 64, 2, long long>(__VA_ARGS__); break;  \
            default: return DLRM_E_MODE;                                                                             \
        }                                                                                                            \
    } while (0)
