// interact_qr.hip — fused lookup + pairwise-dot interaction, forward AND backward, over quotient-remainder (QR) embedding tables, gfx950.
//
// Replaces, for batches with ONE lookup per bag: dlrm_emb_fwd_qr + dlrm_interact_fwd (forward) and dlrm_interact_bwd over the pooled
//   [B, T*D] fp32 buffer + dlrm_emb_qr_bwd_split (backward).  Neither that buffer, nor its gradient, nor the [B, 2*Tq*D] pooled sums the
//   two-kernel forward keeps for its backward are written or read, and nothing has to live from forward to backward except x: the backward
//   fetches the weight_q / weight_r rows again.  A table list may mix QR tables (collisions > 0) and plain fp32 tables (collisions == 0).
//
// Contract (include/dlrm_hip.h):
//   forward : R is BIT-IDENTICAL to dlrm_emb_fwd_qr (saved = NULL) into a feature buffer + dlrm_interact_fwd, modes 0 / 1 / 2;
//   backward: dx is BIT-IDENTICAL to dlrm_interact_bwd over (x, that buffer), gout [B, Tv*D] to dlrm_emb_qr_bwd_split applied to that call's
//             embedding gradient and the sums the forward would have saved (virtual table list: q then r for a QR table, Tv = T + Tq).
//   * element = fmaf(1, Wq[q], +0) op fmaf(1, Wr[r], +0), op = * or +, each rounded once — the lookup's arithmetic from zero accumulators
//     (emb_qr.hip), so -0.0 in a table row becomes +0.0 before the composition; fmaf(1, W[id], +0) for a plain table.  q, r: qr_split
//     (qr_split.h, shared with emb_qr.hip: the FLOAT32 quotient).  A lookup emb_fwd_qr skips gives a row of +0.0 and is reported; its gout
//     rows are dout * (+0) (MULT) / dout (ADD), as the two-kernel form writes them;
//   * products = the summation order of the D = 128 interaction kernels (interact.hip): the composed rows go through registers into the
//     wave-private swizzled fp32 LDS image of interact_{fwd,bwd}_dma_kernel (16-byte slot q of row r holds quad q ^ (r & 15); rows F.. are
//     zero) and those kernels' fragment-read / MFMA / store sections run on it unchanged (as csrc/interact_bf16.hip).
//
// Row fetch: an fp32 row of D = 128 is 512 bytes; a lane owns 4 columns = ONE 16-byte load, 32 lanes cover a row, a wave fetches 2 rows per
//   pass, ceil((F - 1) / 2) <= 13 passes per sample; a QR row costs a second load, of weight_r, which is c rows (2 KiB at c = 4) and is read
//   through the caches like emb_qr.hip does — nothing is staged, so no shape depends on c.  Lane f (1 <= f < F) owns feature f's selector:
//   it loads idx[f][s] and off[f][s], checks them, splits the id and hands q and r to the 32 lanes of that row by lane shuffle.
//
// Pipeline (per wave, four waves per workgroup = one per SIMD, no barrier in the sample loop, two images per wave): at the top of sample n
//   the rows (and x, and the dR row) of sample n + 1 are issued into registers from selectors that were loaded during sample n - 1, then the
//   selectors of sample n + 2 are issued; sample n is multiplied from image[cur]; only then are the registers composed and written into
//   image[cur ^ 1] and the selectors checked and split.  Look-ahead past the last sample is clamped to B - 1.  Every memory operation is an
//   ordinary global load / store or LDS access that the compiler counts: no inline-asm loads, no LDS-DMA, no hand-placed waits.
//
// Backward, the virtual table list: the interaction kernel's row store of feature f goes to the q slot of table f - 1 in gout.  ADD: the same
//   row is stored a second time D columns further (the r slot).  MULT: interact_qr_mult_kernel, a second launch of the same call behind
//   the same predicate, gathers Wq[q] and Wr[r] again (half a wave per sample and table) and turns the row in place into dout * sr | dout * sq.
//   Keeping both components of every row in LDS beside the composed image instead would double the images: 281 KiB at F > 16, more than
//   the 160 KiB of a CU.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, 64-bit ids / 32-bit ids where they differ; no static
//   LDS, the dynamic LDS of a workgroup is what qr_lds() returns):
//                                     VGPRs      AGPRs      SGPRs  scratch  dynamic LDS
//   interact_fwd_qr_kernel<1, IT>     202 / 204     8        106      0      67328 B   (F <= 16: two workgroups per CU)
//   interact_fwd_qr_kernel<2, IT>     256        88 / 90     106      0     132864 B   (one workgroup per CU)
//   interact_bwd_qr_kernel<1, IT>     221          16        106      0      83712 B   (F <= 16: one workgroup per CU)
//   interact_bwd_qr_kernel<2, IT>     256       133 / 132    106      0     149248 B   (one workgroup per CU)
//   interact_qr_mult_kernel<IT>        30 / 28      0       44 / 36   0          0 B
//   One wave per SIMD may use 512 registers (the NB = 2 instantiations keep the 104 row registers of the next sample partly in AGPRs), so
//   registers limit no launch; LDS bounds the workgroups per CU, as the last column says.  Scratch is 0: the kernarg tables are copied to
//   LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch), and the x quad of lanes >= 32 is
//   an assignment under `if`, not a ?: between a load and a zero constant.  The only flat_* instructions are the volatile stores of the
//   error report.
#include "common.h"
#include "qr_split.h"

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
constexpr int BI_SRCB = BI_D * 4;           // bytes of a table row (fp32)
constexpr int BI_DRB = 2048;                // dR row image of the backward (as the fp32 gather backward); its last word stays zero
constexpr unsigned BI_BAD = 0xFFFFFFFFu;    // row selector of an out-of-range id (tables have at most 0xFFFFFFFF rows: never a valid row)

// feature f >= 1 is table f - 1; slot 0 is unused (feature 0 = x)
struct BGatherArgs {
    const void* w[BI_MAXF];                 // weight_q of a QR table, the rows of a plain one
    const void* wr[BI_MAXF];                // weight_r (nullptr: plain table)
    const void* idx[BI_MAXF];
    const void* off[BI_MAXF];               // bag starts: verified to be 0, 1, 2, ... (one lookup per bag)
    long long   rows[BI_MAXF];              // n: the categories of the table
    long long   rows_q[BI_MAXF];            // ceil(n / c) (plain: n)
    int         coll[BI_MAXF];              // collisions (0: plain table)
    int         vs[BI_MAXF];                // backward: virtual slot of the table (of its q component) in gout
    long long*  err;
    DlrmPred    pred;
};

// fma(1, v, +0): dlrm_emb_fwd_qr's sum of a bag of one row (-0.0 becomes +0.0)
__device__ __forceinline__ float bag1(float v) { return __builtin_fmaf(1.0f, v, 0.f); }
__device__ __forceinline__ float4 bag1(const floatx4& v) { return make_float4(bag1(v.x), bag1(v.y), bag1(v.z), bag1(v.w)); }

template <int NB> struct BPasses { static constexpr int N = NB == 1 ? 8 : 13; };     // rows 1 .. 16 NB - 1 (F <= 27), two per pass

// what the owner lane hands to the lanes of a row: the weight_q row (BI_BAD: the zero row) and the weight_r row
struct QRow { unsigned q, r; };

// what a lane keeps across the sample loop
template <int NP>
struct BLane {
    const gchar* base[NP];      // the lane's 16 bytes of row 0 of weight_q (plain: of the table) behind image row 1 + 2 p + (lane >> 5)
    const gchar* baser[NP];     // the same of weight_r
    unsigned wofs[NP];          // byte offset of the lane's 16-byte slot inside the image
    bool on[NP];                // that row is a feature (< F)
    bool qr[NP];                // ... of a QR table
    const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
    const gchar* osrc;
    long long rows, rows_q;
    int coll;
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

// the owner lane's checks and the index split (emb_qr.hip's: a lookup dlrm_emb_fwd_qr skips selects the zero row and is reported)
template <typename IT, int NP>
__device__ __forceinline__ QRow sel_resolve(const BLane<NP>& bl, const BSel<IT>& sel, long long s, int lane, long long* err, bool live = true) {
    QRow o; o.q = BI_BAD; o.r = 0u;
    if (bl.own && live) {                   // (not live: look-ahead past the last sample — the zero row, nothing reported)
        const long long id = (long long)sel.id, of = (long long)sel.off;
        if (of != s) dlrm_report_bad_index(err, lane - 1, -(of + 1), -1);               // not a one-lookup-per-bag batch (rows = -1 marks it)
        long long q = id, r = 0;
        const bool ok = bl.coll ? qr_split(id, bl.rows, bl.coll, bl.rows_q, &q, &r) : dlrm_index_ok(id, bl.rows);
        if (!ok) dlrm_report_bad_index(err, lane - 1, id, bl.rows);
        else { o.q = (unsigned)q; o.r = (unsigned)r; }
    }
    return o;
}

// the rows of one sample, as loaded: weight_q (or the plain table) and weight_r, one 16-byte quad per lane and pass
template <int NP>
struct QRegs { floatx4 q[NP], r[NP]; };

// row loads of one sample into registers: NP passes, two rows per pass, nothing waits here.  weight_r is c rows: it stays in the caches
template <int NP>
__device__ __forceinline__ void rows_issue(QRegs<NP>& v, const BLane<NP>& bl, const QRow& sel, int lane) {
    const int g = lane >> 5;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const unsigned mq = (unsigned)__shfl((int)sel.q, 1 + 2 * p + g, 64);      // (1 + 2 p + g <= 26: always a lane of this wave)
        const unsigned mr = (unsigned)__shfl((int)sel.r, 1 + 2 * p + g, 64);
        v.q[p] = (floatx4){0.f, 0.f, 0.f, 0.f};
        v.r[p] = (floatx4){0.f, 0.f, 0.f, 0.f};
        if (bl.on[p] && mq != BI_BAD) {
            v.q[p] = *(const gfloatx4*)(bl.base[p] + (unsigned long long)mq * BI_SRCB);       // 64-bit byte offset
            if (bl.qr[p]) v.r[p] = *(const gfloatx4*)(bl.baser[p] + (unsigned long long)mr * BI_SRCB);
        }
    }
}

// compose and write: sq = 0 + Wq[q], sr = 0 + Wr[r], one multiply / add — dlrm_emb_fwd_qr's element for a bag of one lookup (a skipped
// lookup is 0 * 0 or 0 + 0 = +0)
template <int NP>
__device__ __forceinline__ void image_write(char* img, const QRegs<NP>& v, const BLane<NP>& bl, const float4& xv, int lane, int op_add) {
    if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (bl.on[p]) {
            float4 y = bag1(v.q[p]);
            if (bl.qr[p]) {
                const float4 sr = bag1(v.r[p]);
                if (op_add) y = make_float4(y.x + sr.x, y.y + sr.y, y.z + sr.z, y.w + sr.w);
                else        y = make_float4(y.x * sr.x, y.y * sr.y, y.z * sr.z, y.w * sr.w);
            }
            *(float4*)(img + bl.wofs[p]) = y;
        }
    }
}

constexpr int BI_NTAB = 7;                  // tables of the argument block kept in LDS, BI_MAXF 8-byte words each

// the kernarg tables into LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch):
// [0] w  [1] wr  [2] idx  [3] off  [4] rows  [5] rows_q  [6] coll | vs << 32
__device__ __forceinline__ void args_to_lds(const BGatherArgs& ba, long long* tab, int F) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int f = 1; f < BI_MAXF; ++f)
        if (tid == f && f < F) {
            tab[0 * BI_MAXF + f] = (long long)ba.w[f];   tab[1 * BI_MAXF + f] = (long long)ba.wr[f];
            tab[2 * BI_MAXF + f] = (long long)ba.idx[f]; tab[3 * BI_MAXF + f] = (long long)ba.off[f];
            tab[4 * BI_MAXF + f] = ba.rows[f];           tab[5 * BI_MAXF + f] = ba.rows_q[f];
            tab[6 * BI_MAXF + f] = (long long)(((unsigned long long)(unsigned)ba.vs[f] << 32) | (unsigned)ba.coll[f]);
        }
}

template <int NP>
__device__ __forceinline__ void lane_init(BLane<NP>& bl, const long long* tab, int F, int lane) {
    const int g = lane >> 5, li = lane & 31;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = 1 + 2 * p + g;
        bl.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
        bl.qr[p] = bl.on[p] && (int)(tab[6 * BI_MAXF + row] & 0xFFFFFFFFLL) != 0;
        bl.base[p] = bl.on[p] ? (const gchar*)tab[0 * BI_MAXF + row] + 16 * li : nullptr;
        bl.baser[p] = bl.qr[p] ? (const gchar*)tab[1 * BI_MAXF + row] + 16 * li : nullptr;
        bl.wofs[p] = row * BI_ROWB + ((li ^ (row & 15)) * 16);
    }
    bl.own = lane >= 1 && lane < F;
    bl.qsrc = bl.own ? (const gchar*)tab[2 * BI_MAXF + lane] : nullptr;
    bl.osrc = bl.own ? (const gchar*)tab[3 * BI_MAXF + lane] : nullptr;
    bl.rows = bl.own ? tab[4 * BI_MAXF + lane] : 0;
    bl.rows_q = bl.own ? tab[5 * BI_MAXF + lane] : 0;
    bl.coll = bl.own ? (int)(tab[6 * BI_MAXF + lane] & 0xFFFFFFFFLL) : 0;
}

// -------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------
template <int NB, typename IT>          // NB = 16-row tiles of the image: 1 (F <= 16) or 2
__global__ __launch_bounds__(256) void interact_fwd_qr_kernel(BGatherArgs ba, const float* __restrict__ x, long long x_ld, long long B,
                                                                int F, int self, int op_add, float* __restrict__ R, long long ldr) {
    if (ba.pred.skip()) return;                              // (the two-kernel form runs instead)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = BPasses<NB>::N;
    constexpr int IMGB = 16 * NB * BI_ROWB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + BI_NTAB * BI_MAXF) + (size_t)wave * 2 * IMGB;

    args_to_lds(ba, tab, F);
    for (int e = lane; e < 2 * IMGB / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);      // rows F.. stay zero
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    BLane<NP> bl;
    lane_init<NP>(bl, tab, F, lane);

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
    QRow idun;
    {
        const QRow idu = sel_resolve<IT, NP>(bl, sel_load<IT, NP>(bl, b), b, lane, ba.err);
        QRegs<NP> v;
        rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;                                  // (not a ?: of two lvalues: that selects between ADDRESSES and puts zero4 into scratch)
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const long long s1 = b + b_stride;
        const BSel<IT> sel1 = sel_load<IT, NP>(bl, s1 < B ? s1 : last);
        image_write<NP>(img0, v, bl, xv, lane, op_add);
        idun = sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err, s1 < B);
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end: its image is written and never multiplied): rows out now from the selectors that were
        // loaded and checked one sample ago, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        QRegs<NP> vn;
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
        image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane, op_add);
        idun = sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err, s2 < B);

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
// backward: dT = (dZ + dZ^T) . T per sample (interact_bwd_dma_kernel, non-UPD), T composed from the weight_q / weight_r rows
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
__global__ __launch_bounds__(256) void interact_bwd_qr_kernel(BGatherArgs ba, const float* __restrict__ x, long long x_ld, long long B,
                                                                int F, int self, int op_add, const float* __restrict__ dR, long long ldr,
                                                                float* __restrict__ dx, long long dx_ld, float* __restrict__ dE, long long dE_ld) {
    if (ba.pred.skip()) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = BPasses<NB>::N;
    constexpr int IMGB = 16 * NB * BI_ROWB;
    constexpr int DRB = BI_DRB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    long long* tab = (long long*)lds;
    char* img0 = (char*)(tab + BI_NTAB * BI_MAXF) + (size_t)wave * (2 * IMGB + 2 * DRB);
    char* drow0 = img0 + 2 * IMGB;

    args_to_lds(ba, tab, F);
    for (int e = lane; e < (2 * IMGB + 2 * DRB) / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * 4;
    long long b = (long long)blockIdx.x * 4 + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    BLane<NP> bl;
    lane_init<NP>(bl, tab, F, lane);
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
    // destination rows of this lane: i = 16 r + 4 g + q — feature 0 is dx, feature f >= 1 the columns of its VIRTUAL slot in gout (dE): the
    // q component of a QR table (ADD: the r component, D columns further, gets the same row — dupbits; MULT: interact_qr_mult_kernel
    // multiplies in place afterwards).  GLOBAL pointers.
    gchar* orow[NB][4];
    long long ostep[NB][4];
    unsigned rowbits = 0u, dupbits = 0u;
#pragma unroll
    for (int r = 0; r < NB; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 16 * r + 4 * g + q;
            if (i < F) rowbits |= 1u << (4 * r + q);
            const long long cv = (i >= 1 && i < F) ? tab[6 * BI_MAXF + i] : 0;           // coll | vs << 32
            if (op_add && (int)(cv & 0xFFFFFFFFLL) != 0) dupbits |= 1u << (4 * r + q);
            const long long ld = i == 0 ? dx_ld : dE_ld;
            float* base = i == 0 ? dx : dE + (cv >> 32) * BI_D;
            orow[r][q] = (i < F) ? (gchar*)(base + b * ld + 4 * li) : nullptr;
            ostep[r][q] = b_stride * ld * 4;
        }

    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's images, and the second sample's (checked) selectors
    QRow idun;
    {
        const QRow idu = sel_resolve<IT, NP>(bl, sel_load<IT, NP>(bl, b), b, lane, ba.err);
        QRegs<NP> v;
        rows_issue<NP>(v, bl, idu, lane);
        float4 xv = zero4;                                  // (not a ?: of two lvalues: that selects between ADDRESSES and puts zero4 into scratch)
        if (lane < 32) xv = *(const float4*)(x + b * x_ld + 4 * lane);
        const DrRegs d = dr_load(dR + b * ldr, rowb, lane);
        const long long s1 = b + b_stride;
        const BSel<IT> sel1 = sel_load<IT, NP>(bl, s1 < B ? s1 : last);
        image_write<NP>(img0, v, bl, xv, lane, op_add);
        dr_write(drow0, d, rowb, lane);
        idun = sel_resolve<IT, NP>(bl, sel1, s1, lane, ba.err, s1 < B);
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end): rows, x and the dR row out now, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        const long long n1 = s1 < B ? s1 : last;
        QRegs<NP> vn;
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
                        if ((dupbits >> (4 * r + q)) & 1u) *(gfloatx4*)(orow[r][q] + dq * 256 + BI_ROWB) = (floatx4){v.x, v.y, v.z, v.w};
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) if ((rowbits >> (4 * r + q)) & 1u) orow[r][q] += ostep[r][q];

        // only now are the next sample's registers touched (see the forward kernel)
        image_write<NP>(img0 + (cur ^ 1) * IMGB, vn, bl, xn, lane, op_add);
        dr_write(drow0 + (cur ^ 1) * DRB, dn, rowb, lane);
        idun = sel_resolve<IT, NP>(bl, seln, s2, lane, ba.err, s2 < B);
        cur ^= 1;
    }
}

// -------------------------------------------------------------------------------------------
// backward, MULT: gout[b, v] = dout * sr, gout[b, v + 1] = dout * sq, in place over the dout rows interact_bwd_qr_kernel left in the q
// slots.  The two rows are gathered again (weight_q from HBM / L2, weight_r from the caches); no selector is reported twice.  Half a wave
// per (sample, table), a 16-byte quad per lane; blockIdx.y = feature - 1.
// -------------------------------------------------------------------------------------------
template <typename IT>
__global__ __launch_bounds__(256) void interact_qr_mult_kernel(BGatherArgs ba, long long B, float* __restrict__ gout, long long gout_ld) {
    if (ba.pred.skip()) return;
    const int f = 1 + blockIdx.y;                       // workgroup-uniform: the kernarg tables are read with scalar loads
    const int c = ba.coll[f];
    if (c == 0) return;                                 // a plain table: its row is final
    const IT* __restrict__ idx = (const IT*)ba.idx[f];
    const gchar* Wq = (const gchar*)ba.w[f];
    const gchar* Wr = (const gchar*)ba.wr[f];
    const long long n = ba.rows[f], rows_q = ba.rows_q[f];
    const int li = threadIdx.x & 31;
    const long long step = (long long)gridDim.x * 8;
    for (long long b = (long long)blockIdx.x * 8 + (threadIdx.x >> 5); b < B; b += step) {
        long long q = 0, r = 0;
        const bool ok = qr_split((long long)idx[b], n, c, rows_q, &q, &r);
        floatx4 vq = (floatx4){0.f, 0.f, 0.f, 0.f}, vr = vq;          // a skipped lookup: the sums are +0
        if (ok) {
            vq = *(const gfloatx4*)(Wq + (unsigned long long)q * BI_SRCB + 16 * li);
            vr = *(const gfloatx4*)(Wr + (unsigned long long)r * BI_SRCB + 16 * li);
        }
        float* o = gout + b * gout_ld + (long long)ba.vs[f] * BI_D + 4 * li;
        const float4 d = *(const float4*)o;
        const float4 sq = bag1(vq), sr = bag1(vr);
        *(float4*)o = make_float4(d.x * sr.x, d.y * sr.y, d.z * sr.z, d.w * sr.w);
        *(float4*)(o + BI_D) = make_float4(d.x * sq.x, d.y * sq.y, d.z * sq.z, d.w * sq.w);
    }
}

constexpr int BI_WAVES = 4;          // one per SIMD

size_t qr_lds(int nb, bool bwd) {
    return BI_NTAB * BI_MAXF * sizeof(long long) + (size_t)BI_WAVES * (2 * (size_t)(16 * nb * BI_ROWB) + (bwd ? 2 * (size_t)BI_DRB : 0));
}
long long qr_grid(long long B, size_t lds) {
    const long long per_cu = (160 * 1024) / (long long)lds >= 2 ? 2 : 1;
    long long nb = (B + BI_WAVES - 1) / BI_WAVES;
    if (nb > 256 * per_cu) nb = 256 * per_cu;
    return nb;
}

template <int NB, typename IT>
void launch_fwd(const BGatherArgs& ba, const float* x, long long x_ld, long long B, int F, int self, int op_add, float* R, long long ldr,
                hipStream_t st) {
    const size_t lds = qr_lds(NB, false);
    (void)hipFuncSetAttribute((const void*)interact_fwd_qr_kernel<NB, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((interact_fwd_qr_kernel<NB, IT>), dim3((unsigned)qr_grid(B, lds)), dim3(64 * BI_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, op_add, R, ldr);
}

template <int NB, typename IT>
void launch_bwd(const BGatherArgs& ba, const float* x, long long x_ld, long long B, int F, int self, int op_add, const float* dR, long long ldr,
                float* dx, long long dx_ld, float* dE, long long dE_ld, hipStream_t st) {
    const size_t lds = qr_lds(NB, true);
    (void)hipFuncSetAttribute((const void*)interact_bwd_qr_kernel<NB, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((interact_bwd_qr_kernel<NB, IT>), dim3((unsigned)qr_grid(B, lds)), dim3(64 * BI_WAVES), lds, st, ba, x, x_ld, B, F,
                       self, op_add, dR, ldr, dx, dx_ld, dE, dE_ld);
}

// the argument block shared by both entry points; 0 or a DLRM_E_* code.  *n_qr: the QR tables of the call (Tv = F - 1 + *n_qr)
int fill_args(BGatherArgs& ba, int F, const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
              const int32_t* collisions_host, const void* const* index_host, const void* const* offsets_host, int64_t* err,
              const int32_t* pred_flag, int pred_nonzero, int* n_qr) {
    ba.err = (long long*)err;
    ba.pred = DlrmPred{(const int*)pred_flag, pred_nonzero};
    int vslot = 0;
    *n_qr = 0;
    for (int f = 0; f < BI_MAXF; ++f) {
        const bool live = f >= 1 && f < F;
        const int t = live ? f - 1 : (F > 1 ? 0 : -1);                   // unused slots repeat table 0 (never dereferenced)
        const int c = t >= 0 ? collisions_host[t] : 0;
        ba.w[f] = t >= 0 ? weight_host[t] : nullptr;
        ba.wr[f] = (t >= 0 && c > 0) ? weight_r_host[t] : nullptr;
        ba.idx[f] = t >= 0 ? index_host[t] : nullptr;
        ba.off[f] = t >= 0 ? offsets_host[t] : nullptr;
        ba.rows[f] = t >= 0 ? rows_host[t] : 0;
        ba.rows_q[f] = (t >= 0 && c > 0) ? (rows_host[t] + c - 1) / c : ba.rows[f];
        ba.coll[f] = c;
        ba.vs[f] = live ? vslot : 0;
        if (live) {
            if (!ba.w[f] || !ba.idx[f] || !ba.off[f] || ba.rows[f] <= 0 || c < 0 || (c > 0 && !ba.wr[f])) return DLRM_E_ARG;
            if (ba.rows_q[f] > 0xFFFFFFFFLL) return DLRM_E_RANGE;         // row selectors travel as 32-bit values inside the kernels
            if (!dlrm_aligned16(ba.w[f]) || (c > 0 && !dlrm_aligned16(ba.wr[f]))) return DLRM_E_MODE;      // a lane's 4 columns are one 16-byte load
            vslot += c > 0 ? 2 : 1;
            *n_qr += c > 0;
        }
    }
    return 0;
}

}  // namespace

extern "C" int dlrm_interact_gather_qr_ok(int F, int D) {
    return (D == BI_D && F < BI_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                           const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
                                           const int32_t* collisions_host, int op,
                                           const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                           int self_interaction, float* R, int64_t ldr, int64_t* err,
                                           const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !R) return DLRM_E_ARG;
    if (F > 1 && (!weight_host || !weight_r_host || !rows_host || !collisions_host || !index_host || !offsets_host)) return DLRM_E_ARG;
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!dlrm_interact_gather_qr_ok(F, D)) return DLRM_E_MODE;
    if (self_interaction < 0 || self_interaction > 2) return DLRM_E_MODE;     // 0 tril, 1 tril + diagonal, 2 torchrec triu order
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D) return DLRM_E_ARG;
    BGatherArgs ba;
    int n_qr = 0;
    const int rc = fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag,
                             pred_nonzero, &n_qr);
    if (rc) return rc;
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(R) || ldr % 4 != 0) return DLRM_E_MODE;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    const int op_add = op == DLRM_QR_ADD;
    if (F <= 16) {
        if (idx_bits == 64) launch_fwd<1, long long>(ba, x, x_ld, B, F, self, op_add, R, ldr, st);
        else                launch_fwd<1, int>(ba, x, x_ld, B, F, self, op_add, R, ldr, st);
    } else {
        if (idx_bits == 64) launch_fwd<2, long long>(ba, x, x_ld, B, F, self, op_add, R, ldr, st);
        else                launch_fwd<2, int>(ba, x, x_ld, B, F, self, op_add, R, ldr, st);
    }
    DLRM_LAUNCH_CHECK();
    return 0;
}

extern "C" int dlrm_interact_bwd_gather_qr(int64_t B, int F, int D, const float* x, int64_t x_ld,
                                           const void* const* weight_host, const void* const* weight_r_host, const int64_t* rows_host,
                                           const int32_t* collisions_host, int op,
                                           const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                           int self_interaction, const float* dR, int64_t ldr,
                                           float* dx, int64_t dx_ld, float* gout, int64_t gout_ld, int64_t* err,
                                           const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !dR || !dx) return DLRM_E_ARG;
    if (F > 1 && (!weight_host || !weight_r_host || !rows_host || !collisions_host || !index_host || !offsets_host || !gout)) return DLRM_E_ARG;
    if (op != DLRM_QR_MULT && op != DLRM_QR_ADD) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!dlrm_interact_gather_qr_ok(F, D)) return DLRM_E_MODE;
    // bits 0-1 as the forward; bit 2 (DLRM_INTERACT_RELU_X): x is the output of a ReLU and dx is multiplied by [x > 0]
    if (self_interaction < 0 || self_interaction > 7 || (self_interaction & 3) > 2) return DLRM_E_MODE;
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D || dx_ld < D) return DLRM_E_ARG;
    BGatherArgs ba;
    int n_qr = 0;
    const int rc = fill_args(ba, F, weight_host, weight_r_host, rows_host, collisions_host, index_host, offsets_host, err, pred_flag,
                             pred_nonzero, &n_qr);
    if (rc) return rc;
    if (F > 1 && gout_ld < (int64_t)(F - 1 + n_qr) * D) return DLRM_E_ARG;     // the virtual table list: Tv = T + Tq
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(dR) || ldr % 4 != 0 || !dlrm_aligned16(dx) || dx_ld % 4 != 0) return DLRM_E_MODE;
    if (F > 1 && (!dlrm_aligned16(gout) || gout_ld % 4 != 0)) return DLRM_E_MODE;
    if (ldr * 4 >= BI_DRB) return DLRM_E_MODE;                 // (strictly: the dR image's last word stays zero)
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 7;
    const int op_add = op == DLRM_QR_ADD;
    if (F <= 16) {
        if (idx_bits == 64) launch_bwd<1, long long>(ba, x, x_ld, B, F, self, op_add, dR, ldr, dx, dx_ld, gout, gout_ld, st);
        else                launch_bwd<1, int>(ba, x, x_ld, B, F, self, op_add, dR, ldr, dx, dx_ld, gout, gout_ld, st);
    } else {
        if (idx_bits == 64) launch_bwd<2, long long>(ba, x, x_ld, B, F, self, op_add, dR, ldr, dx, dx_ld, gout, gout_ld, st);
        else                launch_bwd<2, int>(ba, x, x_ld, B, F, self, op_add, dR, ldr, dx, dx_ld, gout, gout_ld, st);
    }
    DLRM_LAUNCH_CHECK();
    if (!op_add && n_qr > 0) {
        long long nb = (B + 7) / 8; if (nb > 4096) nb = 4096;
        dim3 grid((unsigned)nb, (unsigned)(F - 1), 1), block(256, 1, 1);
        if (idx_bits == 64) hipLaunchKernelGGL(interact_qr_mult_kernel<long long>, grid, block, 0, st, ba, (long long)B, gout, (long long)gout_ld);
        else                hipLaunchKernelGGL(interact_qr_mult_kernel<int>, grid, block, 0, st, ba, (long long)B, gout, (long long)gout_ld);
        DLRM_LAUNCH_CHECK();
    }
    return 0;
}
