// interact_bf16.hip — fused lookup + pairwise-dot interaction, forward AND backward, over bfloat16 embedding tables, gfx950.
//
// Replaces, for batches with ONE lookup per bag and no per-sample weights: dlrm_emb_fwd_bf16 + dlrm_interact_fwd (forward) and
//   dlrm_interact_bwd over the pooled [B, T*D] fp32 buffer (backward).  That buffer is neither written nor read, and nothing has to live
//   from forward to backward except x: the backward fetches the bf16 rows again.
//
// Contract (include/dlrm_hip.h):
//   forward : R is BIT-IDENTICAL to dlrm_emb_fwd_bf16 (psw_host = NULL) into a feature buffer + dlrm_interact_fwd, modes 0 / 1 / 2;
//   backward: dx, dE are BIT-IDENTICAL to dlrm_interact_bwd over (x, that buffer); dE[b, t*D : (t+1)*D] is the gradient row of table t.
//   * element = fmaf(1.0f, upcast(bits), +0.0f) — the lookup's arithmetic from a zero accumulator (emb_bf16.hip), so -0.0 becomes +0.0;
//     an out-of-range id gives a row of +0.0 and is reported (NOT row 0, which the fp32 fused kernels read); its gradient row is written
//     like any other;
//   * products = the summation order of the D = 128 interaction kernels (interact.hip): both follow from widening the rows into the
//     wave-private swizzled fp32 LDS image of interact_{fwd,bwd}_dma_kernel (16-byte slot q of row r holds quad q ^ (r & 15); rows F..
//     are zero) and running those kernels' fragment-read / MFMA / store sections on it unchanged.
//
// Row fetch: a bf16 row of D = 128 is 256 bytes; a lane owns 8 columns = ONE 16-byte load, 16 lanes cover a row, a wave fetches 4 rows per
//   pass, ceil((F - 1) / 4) <= 7 passes per sample.  Lane f (1 <= f < F) owns feature f's selector: it loads idx[f][s] and off[f][s], checks
//   them and hands the row number to the 16 lanes of that row by lane shuffle.  Widening is a 16-bit shift / mask: 2 VALU per pair of
//   elements plus the fma.  Feature 0 (x) is one float4 load in lanes 0..31; the backward's dR row is at most two 16-byte loads per lane.
//
// Pipeline (per wave, four waves per workgroup = one per SIMD, no barrier in the sample loop, two images per wave): at the top of sample
//   n the rows (and x, and the dR row) of sample n + 1 are issued into registers from selectors that were loaded during sample n - 1, then
//   the selectors of sample n + 2 are issued; sample n is multiplied from image[cur]; only then are the registers widened and written
//   into image[cur ^ 1] and the selectors checked.  Look-ahead past the last sample is clamped to B - 1.  Every memory operation is an
//   ordinary global load / store or LDS access that the compiler counts: no inline-asm loads, no LDS-DMA, no hand-placed waits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, the same for 32- and 64-bit ids; no static LDS, the
//   dynamic LDS of a workgroup is what bf16_lds() returns):
//                                     VGPRs  AGPRs  SGPRs  scratch  dynamic LDS
//   interact_fwd_bf16_kernel<1, IT>     118      8     90      0      66560 B   (F <= 16: two workgroups per CU)
//   interact_fwd_bf16_kernel<2, IT>     196     24     90      0     132096 B   (one workgroup per CU)
//   interact_bwd_bf16_kernel<1, IT>     128     20     90      0      82944 B   (F <= 16: one workgroup per CU)
//   interact_bwd_bf16_kernel<2, IT>     240     28     92      0     148480 B   (one workgroup per CU)
//   One wave per SIMD may use 512 registers, so none of these limits the launch; LDS does.  Scratch is 0: the kernarg pointer tables are
//   copied to LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch), and the x quad of
//   lanes >= 32 is an assignment under `if`, not a ?: between a load and a zero constant (that selects between two ADDRESSES and keeps the
//   constant in scratch).  The only flat_* instructions are the volatile stores of the error report.
#include "common.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) char gchar;          // pointers rebuilt from integers: tag them global (global_*, not flat_* accesses)
typedef __attribute__((address_space(1))) floatx4 gfloatx4;

// position of the pair (i, j), j <= i, in the flattened interaction output — as interact.hip: bit 0 = with the diagonal, bit 1 = torchrec order
__device__ __forceinline__ int pair_pos(int i, int j, int F, int mode) {
    if (mode & 2) return j * F - j * (j + 1) / 2 + (i - j - 1);
    return ((mode & 1) ? i * (i + 1) / 2 : i * (i - 1) / 2) + j;
}

constexpr int BI_D = 128;
constexpr int BI_MAXF = 32;                 // feature slots of the argument block (dlrm_interact_gather_ok bounds F at 27)
constexpr int BI_ROWB = BI_D * 4;           // bytes of an image row
constexpr int BI_SRCB = BI_D * 2;           // bytes of a table row
constexpr int BI_DRB = 2048;                // dR row image of the backward (as the fp32 gather backward); its last word stays zero
constexpr unsigned BI_BAD = 0xFFFFFFFFu;    // row selector of an out-of-range id (tables have at most 0xFFFFFFFF rows: never a valid row)

// feature f >= 1 is table f - 1; slot 0 is unused (feature 0 = x)
struct BGatherArgs {
    const void* w[BI_MAXF];                 // bf16 rows
    const void* idx[BI_MAXF];
    const void* off[BI_MAXF];               // bag starts: verified to be 0, 1, 2, ... (one lookup per bag)
    long long   rows[BI_MAXF];
    long long*  err;
    DlrmPred    pred;
};

// bf16 -> fp32 is exact: the 16 bits are the high half of the fp32 pattern
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
// fma(1, v, +0): dlrm_emb_fwd_bf16's element for a bag of one row without per-sample weights
__device__ __forceinline__ float bag1(float v) { return __builtin_fmaf(1.0f, v, 0.f); }

template <int NB> struct BPasses { static constexpr int N = NB == 1 ? 4 : 7; };      // rows 1 .. 16 NB - 1 (F <= 27), four per pass

// what a lane keeps across the sample loop
template <int NP>
struct BLane {
    const gchar* base[NP];      // the lane's 16 bytes of row 0 of the table behind image row 1 + 4 p + (lane >> 4)
    unsigned wofs[NP][2];       // byte offsets of the lane's two 16-byte slots inside the image
    bool on[NP];                // that row is a feature (< F)
    const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
    const gchar* osrc;
    long long rows;
    bool own;
};

template <typename IT>
struct BSel { IT id, off; };

template <typename IT, int NP>
__device__ __forceinline__ BSel<IT> sel_load(const BLane<NP>& bl, long long s) {
    BSel<IT> r; r.id = 0; r.off = 0;
    if (bl.own) {
        r.id = *(const __attribute__((address_space(1))) IT*)(bl.qsrc + s * (long long)sizeof(IT));
        r.off = *(const __attribute__((address_space(1))) IT*)(bl.osrc + s * (long long)sizeof(IT));
    }
    return r;
}

// the owner lane's checks (as gather_rows_issue of interact.hip, except that a bad id selects the zero row, as dlrm_emb_fwd_bf16 skips it)
template <typename IT, int NP>
__device__ __forceinline__ unsigned sel_resolve(const BLane<NP>& bl, const BSel<IT>& sel, long long s, int lane, long long* err) {
    unsigned idu = BI_BAD;
    if (bl.own) {
        const long long id = (long long)sel.id, o = (long long)sel.off;
        if (o != s) dlrm_report_bad_index(err, lane - 1, -(o + 1), -1);                 // not a one-lookup-per-bag batch (rows = -1 marks it)
        if (!dlrm_index_ok(id, bl.rows)) dlrm_report_bad_index(err, lane - 1, id, bl.rows);
        else idu = (unsigned)id;
    }
    return idu;
}

// row loads of one sample into registers: NP passes, one 16-byte load each, nothing waits here
template <int NP>
__device__ __forceinline__ void rows_issue(uint4 (&v)[NP], const BLane<NP>& bl, unsigned idu, int lane) {
    const int g = lane >> 4;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const unsigned mine = (unsigned)__shfl((int)idu, 1 + 4 * p + g, 64);      // (1 + 4 p + g <= 28: always a lane of this wave)
        v[p] = make_uint4(0u, 0u, 0u, 0u);
        if (bl.on[p] && mine != BI_BAD) {
            const uintx4 q = *(const __attribute__((address_space(1))) uintx4*)(bl.base[p] + (unsigned long long)mine * BI_SRCB);   // 64-bit byte offset
            v[p] = make_uint4(q.x, q.y, q.z, q.w);
        }
    }
}

template <int NP>
__device__ __forceinline__ void image_write(char* img, const uint4 (&v)[NP], const BLane<NP>& bl, const float4& xv, int lane) {
    if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (bl.on[p]) {
            const uint4 q = v[p];
            *(float4*)(img + bl.wofs[p][0]) = make_float4(bag1(bf_lo(q.x)), bag1(bf_hi(q.x)), bag1(bf_lo(q.y)), bag1(bf_hi(q.y)));
            *(float4*)(img + bl.wofs[p][1]) = make_float4(bag1(bf_lo(q.z)), bag1(bf_hi(q.z)), bag1(bf_lo(q.w)), bag1(bf_hi(q.w)));
        }
    }
}

// the kernarg tables into LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch)
__device__ __forceinline__ void args_to_lds(const BGatherArgs& ba, long long* tw, long long* tq, long long* to, long long* tr, int F) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int f = 1; f < BI_MAXF; ++f)
        if (tid == f && f < F) { tw[f] = (long long)ba.w[f]; tq[f] = (long long)ba.idx[f]; to[f] = (long long)ba.off[f]; tr[f] = ba.rows[f]; }
}

template <int NP>
__device__ __forceinline__ void lane_init(BLane<NP>& bl, const long long* tw, const long long* tq, const long long* to, const long long* tr,
                                          int F, int lane) {
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = 1 + 4 * p + g;
        bl.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
        bl.base[p] = bl.on[p] ? (const gchar*)tw[row] + 16 * li : nullptr;
        bl.wofs[p][0] = row * BI_ROWB + (((2 * li) ^ (row & 15)) * 16);
        bl.wofs[p][1] = row * BI_ROWB + (((2 * li + 1) ^ (row & 15)) * 16);
    }
    bl.own = lane >= 1 && lane < F;
    bl.qsrc = bl.own ? (const gchar*)tq[lane] : nullptr;
    bl.osrc = bl.own ? (const gchar*)to[lane] : nullptr;
    bl.rows = bl.own ? tr[lane] : 0;
}

// -------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------
template <int NB, typename IT>          // NB = 16-row tiles of the image: 1 (F <= 16) or 2
__global__ __launch_bounds__(256) void interact_fwd_bf16_kernel(BGatherArgs ba, const float* __restrict__ x, long long x_ld, long long B,
                                                                int F, int self, float* __restrict__ R, long long ldr) {
    if (ba.pred.skip()) return;                              // (the two-kernel form runs instead)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = BPasses<NB>::N;
    constexpr int IMGB = 16 * NB * BI_ROWB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tw = (long long*)lds;
    long long* tq = tw + BI_MAXF;
    long long* to = tq + BI_MAXF;
    long long* tr = to + BI_MAXF;
    char* img0 = (char*)(tr + BI_MAXF) + (size_t)wave * 2 * IMGB;

    args_to_lds(ba, tw, tq, to, tr, F);
    for (int e = lane; e < 2 * IMGB / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);      // rows F.. stay zero
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    BLane<NP> bl;
    lane_init<NP>(bl, tw, tq, to, tr, F, lane);

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
    unsigned idun;
    {
        const unsigned idu = sel_resolve<IT, NP>(bl, sel_load<IT, NP>(bl, b), b, lane, ba.err);
        uint4 v[NP];
        rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;                                  // (not a ?: of two lvalues: that selects between ADDRESSES and puts zero4 into scratch)
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const long long s1 = b + b_stride;
        const BSel<IT> sel1 = sel_load<IT, NP>(bl, s1 < B ? s1 : last);
        image_write<NP>(img0, v, bl, xv, lane);
        idun = s1 < B ? sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err) : BI_BAD;
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end: its image is written and never multiplied): rows out now from the selectors that were
        // loaded and checked one sample ago, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        uint4 vn[NP];
        rows_issue<NP>(vn, bl, idun, lane);
        float4 xn = zero4;
        if (lane < 32) xn = *(const float4*)(x + (s1 < B ? s1 : last) * x_ld + 4 * lane);
        const BSel<IT> seln = sel_load<IT, NP>(bl, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        // ---- the fragment-read / MFMA section of interact_fwd_dma_kernel (interact.hip) ----
        float4 fr[NB][BI_D / 16];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int s = 0; s < BI_D / 16; ++s)
                fr[r][s] = *(const float4*)(my + (16 * r + li) * BI_ROWB + (((4 * s + g) ^ li) * 16));      // (row & 15) == li
        const float4 xrow = *(const float4*)(my + (lane & 31) * 16);
        __builtin_amdgcn_sched_barrier(0);      // all fragment reads (and the next sample's loads) in front of the first MFMA
        floatx4 acc[NPAIR][2];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) { acc[p][0] = (floatx4){0.f, 0.f, 0.f, 0.f}; acc[p][1] = (floatx4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < BI_D / 16; ++s) {
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
        image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane);
        idun = s2 < B ? sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err) : BI_BAD;

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
// backward: dT = (dZ + dZ^T) . T per sample (interact_bwd_dma_kernel, non-UPD), T widened from the bf16 rows
// -------------------------------------------------------------------------------------------
// the lane's share of a dR row: bytes [1024 c + 16 lane, +16), c < 2, where they lie inside the row (ldr * 4 < BI_DRB)
struct DrRegs { float4 v[BI_DRB / 1024]; };
__device__ __forceinline__ DrRegs dr_load(const float* __restrict__ row, long long rowb, int lane) {
    DrRegs d;
#pragma unroll
    for (int c = 0; c < BI_DRB / 1024; ++c) {
        d.v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((long long)(1024 * c + 16 * lane) < rowb) d.v[c] = *(const float4*)((const char*)row + 1024 * c + 16 * lane);
    }
    return d;
}
__device__ __forceinline__ void dr_write(char* img, const DrRegs& d, long long rowb, int lane) {
#pragma unroll
    for (int c = 0; c < BI_DRB / 1024; ++c)
        if ((long long)(1024 * c + 16 * lane) < rowb) *(float4*)(img + 1024 * c + 16 * lane) = d.v[c];
}

template <int NB, typename IT>
__global__ __launch_bounds__(256) void interact_bwd_bf16_kernel(BGatherArgs ba, const float* __restrict__ x, long long x_ld, long long B,
                                                                int F, int self, const float* __restrict__ dR, long long ldr,
                                                                float* __restrict__ dx, long long dx_ld, float* __restrict__ dE, long long dE_ld) {
    if (ba.pred.skip()) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = BPasses<NB>::N;
    constexpr int IMGB = 16 * NB * BI_ROWB;
    constexpr int DRB = BI_DRB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long long* tw = (long long*)lds;
    long long* tq = tw + BI_MAXF;
    long long* to = tq + BI_MAXF;
    long long* tr = to + BI_MAXF;
    char* img0 = (char*)(tr + BI_MAXF) + (size_t)wave * (2 * IMGB + 2 * DRB);
    char* drow0 = img0 + 2 * IMGB;

    args_to_lds(ba, tw, tq, to, tr, F);
    for (int e = lane; e < (2 * IMGB + 2 * DRB) / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * 4;
    long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    BLane<NP> bl;
    lane_init<NP>(bl, tw, tq, to, tr, F, lane);
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
    // destination rows of this lane: i = 16 r + 4 g + q — feature 0 is dx, feature f >= 1 columns (f - 1) D .. of dE.  GLOBAL pointers.
    gchar* orow[NB][4];
    long long ostep[NB][4];
    unsigned rowbits = 0u;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 16 * r + 4 * g + q;
            if (i < F) rowbits |= 1u << (4 * r + q);
            const long long ld = i == 0 ? dx_ld : dE_ld;
            float* base = i == 0 ? dx : dE + (long long)(i - 1) * BI_D;
            orow[r][q] = (i < F) ? (gchar*)(base + b * ld + 4 * li) : nullptr;
            ostep[r][q] = b_stride * ld * 4;
        }

    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's images, and the second sample's (checked) selectors
    unsigned idun;
    {
        const unsigned idu = sel_resolve<IT, NP>(bl, sel_load<IT, NP>(bl, b), b, lane, ba.err);
        uint4 v[NP];
        rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;                                  // (not a ?: of two lvalues: that selects between ADDRESSES and puts zero4 into scratch)
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const DrRegs d = dr_load(dR + b * ldr, rowb, lane);
        const long long s1 = b + b_stride;
        const BSel<IT> sel1 = sel_load<IT, NP>(bl, s1 < B ? s1 : last);
        image_write<NP>(img0, v, bl, xv, lane);
        dr_write(drow0, d, rowb, lane);
        idun = s1 < B ? sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err) : BI_BAD;
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end): rows, x and the dR row out now, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        const long long n1 = s1 < B ? s1 : last;
        uint4 vn[NP];
        rows_issue<NP>(vn, bl, idun, lane);
        float4 xn = zero4;
        if (lane < 32) xn = *(const float4*)(x + n1 * x_ld + 4 * lane);
        const DrRegs dn = dr_load(dR + n1 * ldr, rowb, lane);
        const BSel<IT> seln = sel_load<IT, NP>(bl, s2 < B ? s2 : last);

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
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) if ((rowbits >> (4 * r + q)) & 1u) orow[r][q] += ostep[r][q];

        // only now are the next sample's registers touched (see the forward kernel)
        image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane);
        dr_write(drow0 + (cur ^ 1) * DRB, dn, rowb, lane);
        idun = s2 < B ? sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err) : BI_BAD;
        cur ^= 1;
    }
}

constexpr int BI_WAVES = 4;          // one per SIMD

size_t bf16_lds(int nb, bool bwd) {
    return 4 * BI_MAXF * sizeof(long long) + (size_t)BI_WAVES * (2 * (size_t)(16 * nb * BI_ROWB) + (bwd ? 2 * (size_t)BI_DRB : 0));
}
long long bf16_grid(long long B, size_t lds) {
    const long long per_cu = (160 * 1024) / (long long)lds >= 2 ? 2 : 1;
    long long nb = (B + BI_WAVES - 1) / BI_WAVES;
    if (nb > 256 * per_cu) nb = 256 * per_cu;
    return nb;
}

template <int NB, typename IT>
void launch_fwd(const BGatherArgs& ba, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, hipStream_t st) {
    const size_t lds = bf16_lds(NB, false);
    (void)hipFuncSetAttribute((const void*)interact_fwd_bf16_kernel<NB, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((interact_fwd_bf16_kernel<NB, IT>), dim3((unsigned)bf16_grid(B, lds)), dim3(64 * BI_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, R, ldr);
}

template <int NB, typename IT>
void launch_bwd(const BGatherArgs& ba, const float* x, long long x_ld, long long B, int F, int self, const float* dR, long long ldr, float* dx,
                long long dx_ld, float* dE, long long dE_ld, hipStream_t st) {
    const size_t lds = bf16_lds(NB, true);
    (void)hipFuncSetAttribute((const void*)interact_bwd_bf16_kernel<NB, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((interact_bwd_bf16_kernel<NB, IT>), dim3((unsigned)bf16_grid(B, lds)), dim3(64 * BI_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, dR, ldr, dx, dx_ld, dE, dE_ld);
}

// the argument block shared by both entry points; 0 or a DLRM_E_* code
int fill_args(BGatherArgs& ba, int F, const void* const* weight_host, const int64_t* rows_host, const void* const* index_host,
              const void* const* offsets_host, int64_t* err, const int32_t* pred_flag, int pred_nonzero) {
    ba.err = (long long*)err;
    ba.pred = DlrmPred{(const int*)pred_flag, pred_nonzero};
    for (int f = 0; f < BI_MAXF; ++f) {
        const int t = (f >= 1 && f < F) ? f - 1 : (F > 1 ? 0 : -1);      // unused slots repeat table 0 (never dereferenced)
        ba.w[f] = t >= 0 ? weight_host[t] : nullptr;
        ba.idx[f] = t >= 0 ? index_host[t] : nullptr;
        ba.off[f] = t >= 0 ? offsets_host[t] : nullptr;
        ba.rows[f] = t >= 0 ? rows_host[t] : 0;
        if (f >= 1 && f < F) {
            if (!ba.w[f] || !ba.idx[f] || !ba.off[f] || ba.rows[f] <= 0) return DLRM_E_ARG;
            if (ba.rows[f] > 0xFFFFFFFFLL) return DLRM_E_RANGE;            // row selectors travel as 32-bit values inside the kernels
            if (!dlrm_aligned16(ba.w[f])) return DLRM_E_MODE;              // a lane's 8 columns are one 16-byte load; rows are 256 bytes apart
        }
    }
    return 0;
}

}  // namespace

extern "C" int dlrm_interact_gather_bf16_ok(int F, int D) {
    return (D == BI_D && F < BI_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                             const void* const* weight_host, const int64_t* rows_host,
                                             const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                             int self_interaction, float* R, int64_t ldr, int64_t* err,
                                             const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !R) return DLRM_E_ARG;
    if (F > 1 && (!weight_host || !rows_host || !index_host || !offsets_host)) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!dlrm_interact_gather_bf16_ok(F, D)) return DLRM_E_MODE;
    if (self_interaction < 0 || self_interaction > 2) return DLRM_E_MODE;     // 0 tril, 1 tril + diagonal, 2 torchrec triu order
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D) return DLRM_E_ARG;
    BGatherArgs ba;
    const int rc = fill_args(ba, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero);
    if (rc) return rc;
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(R) || ldr % 4 != 0) return DLRM_E_MODE;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    if (F <= 16) {
        if (idx_bits == 64) launch_fwd<1, long long>(ba, x, x_ld, B, F, self, R, ldr, st);
        else                launch_fwd<1, int>(ba, x, x_ld, B, F, self, R, ldr, st);
    } else {
        if (idx_bits == 64) launch_fwd<2, long long>(ba, x, x_ld, B, F, self, R, ldr, st);
        else                launch_fwd<2, int>(ba, x, x_ld, B, F, self, R, ldr, st);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_bf16(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                             const void* const* weight_host, const int64_t* rows_host,
                                             const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                             int self_interaction, const float* dR, int64_t ldr,
                                             float* dx, int64_t dx_ld, float* dE, int64_t dE_ld, int64_t* err,
                                             const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !dR || !dx) return DLRM_E_ARG;
    if (F > 1 && (!weight_host || !rows_host || !index_host || !offsets_host || !dE)) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!dlrm_interact_gather_bf16_ok(F, D)) return DLRM_E_MODE;
    // bits 0-1 as the forward; bit 2 (DLRM_INTERACT_RELU_X): x is the output of a ReLU and dx is multiplied by [x > 0]
    if (self_interaction < 0 || self_interaction > 7 || (self_interaction & 3) > 2) return DLRM_E_MODE;
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D || dx_ld < D || (F > 1 && dE_ld < (int64_t)(F - 1) * D)) return DLRM_E_ARG;
    BGatherArgs ba;
    const int rc = fill_args(ba, F, weight_host, rows_host, index_host, offsets_host, err, pred_flag, pred_nonzero);
    if (rc) return rc;
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(dR) || ldr % 4 != 0 || !dlrm_aligned16(dx) || dx_ld % 4 != 0) return DLRM_E_MODE;
    if (F > 1 && (!dlrm_aligned16(dE) || dE_ld % 4 != 0)) return DLRM_E_MODE;
    if (ldr * 4 >= BI_DRB) return DLRM_E_MODE;                 // (strictly: the dR image's last word stays zero)
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 7;
    if (F <= 16) {
        if (idx_bits == 64) launch_bwd<1, long long>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
        else                launch_bwd<1, int>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
    } else {
        if (idx_bits == 64) launch_bwd<2, long long>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
        else                launch_bwd<2, int>(ba, x, x_ld, B, F, self, dR, ldr, dx, dx_ld, dE, dE_ld, st);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}
