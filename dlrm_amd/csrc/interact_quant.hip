// interact_quant.hip — fused lookup + pairwise-dot interaction, forward only, over row-wise QUANTISED embedding tables, gfx950.
//
// Reference call sites replaced: the quantised branch of DLRM_Net.apply_emb (ops.quantized.embedding_bag_{byte,4bit}_rowwise_offsets,
//   dlrm_s_pytorch.py:430-450) followed by DLRM_Net.interact_features, arch_interaction_op == "dot" (dlrm_s_pytorch.py:483-504), for batches
//   with ONE lookup per bag.  The [B, T*D] fp32 pooled buffer that dlrm_emb_fwd_quant writes and dlrm_interact_fwd reads back never exists.
//
// Contract: R is BIT-IDENTICAL to dlrm_emb_fwd_quant (no per-sample weights, one lookup per bag) + dlrm_interact_fwd:
//   * element  = fmaf(1.0f, fmaf(scale, (float)q, bias), +0.0f)      — the lookup's arithmetic from a zero accumulator (emb_quant.hip); the
//                fp16 scale / bias of the 4-bit form convert exactly; an out-of-range id gives a row of +0.0 and is reported;
//   * dot      = the summation order of every version of the interaction kernel (interact.hip): v_mfma_f32_16x16x4_f32, k-step s outermost,
//                element e of the lane's quad = column 16 s + 4 (lane >> 4) + e, even e into one accumulator and odd e into a second one,
//                the two added at the end, lower-triangle tile pairs only.
//   Both follow from dequantising into the wave-private swizzled fp32 LDS image of interact_fwd_dma_kernel (16-byte slot q of row r holds
//   quad q ^ (r & 15); rows F.. are zero) and running its fragment-read / MFMA / store section on it unchanged.
//
// Row fetch.  Packed rows cannot ride the LDS-DMA into an fp32 image; they go through registers.  A lane owns 8 consecutive columns of a
//   row: one 8-byte (8 bits) or 4-byte (4 bits) load of codes plus the row's scale / bias word; 16 lanes cover a row, a wave 4 rows per
//   pass, ceil((F - 1) / 4) <= 7 passes per sample.  Lane f (1 <= f < F) owns feature f's selector: it loads idx[f][s] and off[f][s], checks
//   them and hands the row number to the 16 lanes of that row by ds_bpermute.  Feature 0 (x) is one float4 load in lanes 0..31.
//
// Pipeline (per wave, no barrier in the sample loop): at the top of sample n the rows of sample n + 1 are issued into registers from
//   selectors that were loaded during sample n - 1, then the selectors of sample n + 2 are issued; sample n is multiplied from image[cur];
//   only then are the registers dequantised and written (two ds_write_b128 per pass) into image[cur ^ 1] and the selectors checked; the
//   stores of sample n come last.  The compiler's s_waitcnt sits in front of the dequantise, so ids and rows are in flight for the
//   whole multiplication, and the stores (which vmcnt counts too) drain beside the next sample's loads.  Look-ahead past the last
//   sample is clamped to B - 1.  All loads are ordinary global loads the compiler counts: no hand-placed waits.
//
// Launch shape: four waves per workgroup, one per SIMD, as the fp32 kernel.  What was weighed:
//   * LDS: two 16 NB-row images per wave = 32 KiB (F > 16) -> 4 waves = 128 KiB + tables: one workgroup per CU; a fifth wave would fit but
//     shares a SIMD with another (the fp32 kernel measured 245 vs 211 us with five).  F <= 16: 16 KiB per wave, two workgroups per CU.
//     The staging registers already are a second buffer, so a single image per wave (8 waves in 115 KiB) would be legal; it is not what
//     is built here — the double-buffered form was asked for and is the one measured (profiles/quant_emb/fused_interact_rates.md).
//   * the exposed VALU dequantise: ~3 (8 bits) / 4 (4 bits) VALU per element, 8 elements per lane and pass: ~170-220 VALU per sample
//     beside 96 MFMAs.  With one wave per SIMD nothing else covers it except the MFMA pipe's own latency (the dequantise is independent
//     of the MFMAs in flight and is placed behind them in program order); the sample time is bounded below by the gather latency of one
//     sample per wave either way, which is what the measurement shows (0.239 / 0.247 ms at 8 / 4 bits against 0.513 / 0.498 ms for the two kernels and 0.214 ms for the fp32
//     fused forward, Criteo-Terabyte shapes).
#include "common.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) char gchar;          // pointers rebuilt from integers: tag them global (global_*, not flat_* loads)

// position of the pair (i, j), j <= i, in the flattened interaction output — as interact.hip: bit 0 = with the diagonal, bit 1 = torchrec order
__device__ __forceinline__ int pair_pos(int i, int j, int F, int mode) {
    if (mode & 2) return j * F - j * (j + 1) / 2 + (i - j - 1);
    return ((mode & 1) ? i * (i + 1) / 2 : i * (i - 1) / 2) + j;
}

constexpr int QI_D = 128;
constexpr int QI_MAXF = 32;                 // feature slots of the argument block (dlrm_interact_gather_quant_ok bounds F at 27)
constexpr int QI_ROWB = QI_D * 4;           // bytes of an image row
constexpr unsigned QI_BAD = 0xFFFFFFFFu;    // row selector of an out-of-range id (tables have at most 0xFFFFFFFF rows: never a valid row)

// feature f >= 1 is table f - 1; slot 0 is unused (feature 0 = x)
struct QGatherArgs {
    const void* w[QI_MAXF];                 // packed rows
    const void* idx[QI_MAXF];
    const void* off[QI_MAXF];               // bag starts: verified to be 0, 1, 2, ... (one lookup per bag)
    long long   rows[QI_MAXF];
    long long*  err;
    DlrmPred    pred;
};

__device__ __forceinline__ float f16_bits_to_f32(unsigned h) {
    union { unsigned short u; _Float16 f; } c; c.u = (unsigned short)h; return (float)c.f;
}

// a lane's 8 columns of one packed row, as emb_quant.hip loads them
template <int BITS> struct QRow;
template <> struct QRow<8> { uint2 q; float2 sb; };
template <> struct QRow<4> { unsigned q; unsigned sb; };
__device__ __forceinline__ void q_zero(QRow<8>& v) { v.q = make_uint2(0u, 0u); v.sb = make_float2(0.f, 0.f); }
__device__ __forceinline__ void q_zero(QRow<4>& v) { v.q = 0u; v.sb = 0u; }
// row: start of the packed row; li: the lane's position inside the row (columns 8 li .. 8 li + 7)
__device__ __forceinline__ void q_load(QRow<8>& v, const gchar* row, int li) {
    const uintx2 q = *(const __attribute__((address_space(1))) uintx2*)(row + 8 * li);
    const floatx2 sb = *(const __attribute__((address_space(1))) floatx2*)(row + QI_D);
    v.q = make_uint2(q.x, q.y); v.sb = make_float2(sb.x, sb.y);
}
__device__ __forceinline__ void q_load(QRow<4>& v, const gchar* row, int li) {
    v.q = *(const __attribute__((address_space(1))) unsigned*)(row + 4 * li);
    v.sb = *(const __attribute__((address_space(1))) unsigned*)(row + QI_D / 2);
}
// out[j] = fma(1, fma(scale, q[j], bias), +0): dlrm_emb_fwd_quant's element for a bag of one row without per-sample weights
__device__ __forceinline__ void q_dequant(float (&o)[8], const QRow<8>& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = __builtin_fmaf(1.0f, __builtin_fmaf(v.sb.x, (float)((v.q.x >> (8 * j)) & 0xFFu), v.sb.y), 0.f);
        o[4 + j] = __builtin_fmaf(1.0f, __builtin_fmaf(v.sb.x, (float)((v.q.y >> (8 * j)) & 0xFFu), v.sb.y), 0.f);
    }
}
__device__ __forceinline__ void q_dequant(float (&o)[8], const QRow<4>& v) {
    const float scale = f16_bits_to_f32(v.sb & 0xFFFFu), bias = f16_bits_to_f32(v.sb >> 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = __builtin_fmaf(1.0f, __builtin_fmaf(scale, (float)((v.q >> (4 * j)) & 0xFu), bias), 0.f);
}

template <int NB> struct QPasses { static constexpr int N = NB == 1 ? 4 : 7; };      // rows 1 .. 16 NB - 1 (F <= 27), four per pass

// what a lane keeps across the sample loop
template <int NP>
struct QLane {
    const gchar* base[NP];      // packed rows of the table behind image row 1 + 4 p + (lane >> 4)
    unsigned wofs[NP][2];       // byte offsets of the lane's two 16-byte slots inside the image
    bool on[NP];                // that row is a feature (< F)
    const gchar* qsrc;          // lanes 1 .. F - 1: idx / off of feature `lane`
    const gchar* osrc;
    long long rows;
    bool own;
};

template <typename IT>
struct QSel { IT id, off; };

template <typename IT, int NP>
__device__ __forceinline__ QSel<IT> sel_load(const QLane<NP>& ql, long long s) {
    QSel<IT> r; r.id = 0; r.off = 0;
    if (ql.own) {
        r.id = *(const __attribute__((address_space(1))) IT*)(ql.qsrc + s * (long long)sizeof(IT));
        r.off = *(const __attribute__((address_space(1))) IT*)(ql.osrc + s * (long long)sizeof(IT));
    }
    return r;
}

// the owner lane's checks (as gather_rows_issue of interact.hip, except that a bad id selects the zero row, as dlrm_emb_fwd_quant skips it)
template <typename IT, int NP>
__device__ __forceinline__ unsigned sel_resolve(const QLane<NP>& ql, const QSel<IT>& sel, long long s, int lane, long long* err) {
    unsigned idu = QI_BAD;
    if (ql.own) {
        const long long id = (long long)sel.id, o = (long long)sel.off;
        if (o != s) dlrm_report_bad_index(err, lane - 1, -(o + 1), -1);                 // not a one-lookup-per-bag batch (rows = -1 marks it)
        if (!dlrm_index_ok(id, ql.rows)) dlrm_report_bad_index(err, lane - 1, id, ql.rows);
        else idu = (unsigned)id;
    }
    return idu;
}

// row loads of one sample into registers: NP passes, two loads each, nothing waits here
template <int BITS, int NP>
__device__ __forceinline__ void rows_issue(QRow<BITS> (&v)[NP], const QLane<NP>& ql, unsigned idu, int lane) {
    constexpr unsigned long long RB = BITS == 8 ? QI_D + 8 : QI_D / 2 + 4;
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const unsigned mine = (unsigned)__shfl((int)idu, 1 + 4 * p + g, 64);      // (1 + 4 p + g <= 28: always a lane of this wave)
        q_zero(v[p]);
        if (ql.on[p] && mine != QI_BAD) q_load(v[p], ql.base[p] + (unsigned long long)mine * RB, li);      // 64-bit byte offset
    }
}

template <int BITS, int NP>
__device__ __forceinline__ void image_write(char* img, const QRow<BITS> (&v)[NP], const QLane<NP>& ql, const float4& xv, int lane) {
    if (lane < 32) *(float4*)(img + 16 * lane) = xv;                    // row 0: (row & 15) == 0, slot = quad
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (ql.on[p]) {
            float o[8];
            q_dequant(o, v[p]);
            *(float4*)(img + ql.wofs[p][0]) = make_float4(o[0], o[1], o[2], o[3]);
            *(float4*)(img + ql.wofs[p][1]) = make_float4(o[4], o[5], o[6], o[7]);
        }
    }
}

template <int NB, int BITS, typename IT>          // NB = 16-row tiles of the image: 1 (F <= 16) or 2
__global__ __launch_bounds__(256) void interact_fwd_quant_kernel(QGatherArgs qa, const float* __restrict__ x, long long x_ld, long long B,
                                                                 int F, int self, float* __restrict__ R, long long ldr) {
    if (qa.pred.skip()) return;                              // (the two-kernel form runs instead)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int NP = QPasses<NB>::N;
    constexpr int IMGB = 16 * NB * QI_ROWB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6));
    long long* tw = (long long*)lds;
    long long* tq = tw + QI_MAXF;
    long long* to = tq + QI_MAXF;
    long long* tr = to + QI_MAXF;
    char* img0 = (char*)(tr + QI_MAXF) + (size_t)wave * 2 * IMGB;

    // the kernarg tables into LDS with compile-time kernarg offsets (a lane-indexed read of a by-value struct would go to scratch)
    {
        const int tid = threadIdx.x;
#pragma unroll
        for (int f = 1; f < QI_MAXF; ++f)
            if (tid == f && f < F) { tw[f] = (long long)qa.w[f]; tq[f] = (long long)qa.idx[f]; to[f] = (long long)qa.off[f]; tr[f] = qa.rows[f]; }
    }
    for (int e = lane; e < 2 * IMGB / 16; e += 64) ((float4*)img0)[e] = make_float4(0.f, 0.f, 0.f, 0.f);      // rows F.. stay zero
    __syncthreads();

    const long long b_stride = (long long)gridDim.x * W;
    long long b = (long long)blockIdx.x * W + wave;
    if (b >= B) return;

    const int g = lane >> 4, li = lane & 15;
    QLane<NP> ql;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int row = 1 + 4 * p + g;
        ql.on[p] = row < F;                                   // no lane loads a row for a feature slot >= F
        ql.base[p] = ql.on[p] ? (const gchar*)tw[row] : nullptr;
        ql.wofs[p][0] = row * QI_ROWB + (((2 * li) ^ (row & 15)) * 16);
        ql.wofs[p][1] = row * QI_ROWB + (((2 * li + 1) ^ (row & 15)) * 16);
    }
    ql.own = lane >= 1 && lane < F;
    ql.qsrc = ql.own ? (const gchar*)tq[lane] : nullptr;
    ql.osrc = ql.own ? (const gchar*)to[lane] : nullptr;
    ql.rows = ql.own ? tr[lane] : 0;

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
                opos[r * (r + 1) / 2 + c][q] = ok ? QI_D + pair_pos(i, j, F, self) : -1;
            }
    constexpr int NPAIR = NB * (NB + 1) / 2;
    const long long last = B - 1;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // prologue: the first sample's image, and the second sample's (checked) selectors
    unsigned idun;
    {
        const unsigned idu = sel_resolve<IT, NP>(ql, sel_load<IT, NP>(ql, b), b, lane, qa.err);
        QRow<BITS> v[NP];
        rows_issue<BITS, NP>(v, ql, idu, lane);
        const float4 xv = lane < 32 ? *(const float4*)(x + b * x_ld + 4 * lane) : zero4;
        const long long s1 = b + b_stride;
        const QSel<IT> sel1 = sel_load<IT, NP>(ql, s1 < B ? s1 : last);
        image_write<BITS, NP>(img0, v, ql, xv, lane);
        idun = s1 < B ? sel_resolve<IT, NP>(ql, sel1, s1, lane, qa.err) : QI_BAD;
    }
    int cur = 0;
    for (; b < B; b += b_stride) {
        // the next sample (clamped past the end: its image is written and never multiplied): rows out now from the selectors that were
        // loaded and checked one sample ago, then the selectors two samples ahead
        const long long s1 = b + b_stride, s2 = s1 + b_stride;
        QRow<BITS> vn[NP];
        rows_issue<BITS, NP>(vn, ql, idun, lane);
        const float4 xn = lane < 32 ? *(const float4*)(x + (s1 < B ? s1 : last) * x_ld + 4 * lane) : zero4;
        const QSel<IT> seln = sel_load<IT, NP>(ql, s2 < B ? s2 : last);

        const char* my = img0 + cur * IMGB;
        // ---- the fragment-read / MFMA section of interact_fwd_dma_kernel (interact.hip) ----
        float4 fr[NB][QI_D / 16];
#pragma unroll
        for (int r = 0; r < NB; ++r)
#pragma unroll
            for (int s = 0; s < QI_D / 16; ++s)
                fr[r][s] = *(const float4*)(my + (16 * r + li) * QI_ROWB + (((4 * s + g) ^ li) * 16));      // (row & 15) == li
        const float4 xrow = *(const float4*)(my + (lane & 31) * 16);
        __builtin_amdgcn_sched_barrier(0);      // all fragment reads (and the next sample's loads) in front of the first MFMA
        floatx4 acc[NPAIR][2];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) { acc[p][0] = (floatx4){0.f, 0.f, 0.f, 0.f}; acc[p][1] = (floatx4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int s = 0; s < QI_D / 16; ++s) {
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
        image_write<BITS, NP>(img0 + (cur ^ 1) * IMGB, vn, ql, xn, lane);
        idun = s2 < B ? sel_resolve<IT, NP>(ql, seln, s2, lane, qa.err) : QI_BAD;

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
        for (long long d = QI_D + P + lane; d < ldr; d += 64) Rb[d] = 0.f;
        cur ^= 1;
    }
}

constexpr int QI_WAVES = 4;          // one per SIMD (see the header)

size_t quant_lds(int nb) { return 4 * QI_MAXF * sizeof(long long) + (size_t)QI_WAVES * 2 * (16 * nb * QI_ROWB); }

template <int NB, int BITS, typename IT>
int launch_quant(const QGatherArgs& qa, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, hipStream_t st) {
    const size_t lds = quant_lds(NB);
    const long long per_cu = (160 * 1024) / (long long)lds >= 2 ? 2 : 1;
    long long nb = (B + QI_WAVES - 1) / QI_WAVES;
    if (nb > 256 * per_cu) nb = 256 * per_cu;
    (void)hipFuncSetAttribute((const void*)interact_fwd_quant_kernel<NB, BITS, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((interact_fwd_quant_kernel<NB, BITS, IT>), dim3((unsigned)nb), dim3(64 * QI_WAVES), lds, st, qa, x, x_ld, B, F, self, R, ldr);
    return 0;
}

template <int BITS, typename IT>
int launch_quant_nb(const QGatherArgs& qa, const float* x, long long x_ld, long long B, int F, int self, float* R, long long ldr, hipStream_t st) {
    return F <= 16 ? launch_quant<1, BITS, IT>(qa, x, x_ld, B, F, self, R, ldr, st) : launch_quant<2, BITS, IT>(qa, x, x_ld, B, F, self, R, ldr, st);
}

}  // namespace

extern "C" int dlrm_interact_gather_quant_ok(int F, int D, int bits) {
    return (D == QI_D && (bits == 4 || bits == 8) && F < QI_MAXF && dlrm_interact_gather_ok(F, D)) ? 1 : 0;
}

extern "C" int dlrm_interact_fwd_gather_quant(int64_t B, int F, int D, int bits, const float* x, int64_t x_ld,
                                              const void* const* qweight_host, const int64_t* rows_host,
                                              const void* const* index_host, const void* const* offsets_host, int idx_bits,
                                              int self_interaction, float* R, int64_t ldr, int64_t* err,
                                              const int32_t* pred_flag, int pred_nonzero, void* stream) {
    if (B <= 0 || F <= 0 || D <= 0 || !x || !R) return DLRM_E_ARG;
    if (F > 1 && (!qweight_host || !rows_host || !index_host || !offsets_host)) return DLRM_E_ARG;
    if (idx_bits != 32 && idx_bits != 64) return DLRM_E_MODE;
    if (!dlrm_interact_gather_quant_ok(F, D, bits)) return DLRM_E_MODE;
    if (self_interaction < 0 || self_interaction > 2) return DLRM_E_MODE;     // 0 tril, 1 tril + diagonal, 2 torchrec triu order
    const int P = (self_interaction & 1) ? F * (F + 1) / 2 : F * (F - 1) / 2;
    if (ldr < D + P || x_ld < D) return DLRM_E_ARG;
    QGatherArgs qa;
    qa.err = (long long*)err;
    qa.pred = DlrmPred{(const int*)pred_flag, pred_nonzero};
    const uintptr_t row_align = bits == 8 ? 7u : 3u;       // a lane's codes are one 8-byte / 4-byte load; rows are 136 / 68 bytes apart
    for (int f = 0; f < QI_MAXF; ++f) {
        const int t = (f >= 1 && f < F) ? f - 1 : (F > 1 ? 0 : -1);      // unused slots repeat table 0 (never dereferenced)
        qa.w[f] = t >= 0 ? qweight_host[t] : nullptr;
        qa.idx[f] = t >= 0 ? index_host[t] : nullptr;
        qa.off[f] = t >= 0 ? offsets_host[t] : nullptr;
        qa.rows[f] = t >= 0 ? rows_host[t] : 0;
        if (f >= 1 && f < F) {
            if (!qa.w[f] || !qa.idx[f] || !qa.off[f] || qa.rows[f] <= 0) return DLRM_E_ARG;
            if (qa.rows[f] > 0xFFFFFFFFLL) return DLRM_E_RANGE;            // row selectors travel as 32-bit values inside the kernel
            if (((uintptr_t)qa.w[f]) & row_align) return DLRM_E_MODE;
        }
    }
    if (!dlrm_aligned16(x) || x_ld % 4 != 0 || !dlrm_aligned16(R) || ldr % 4 != 0) return DLRM_E_MODE;
    hipStream_t st = (hipStream_t)stream;
    const int self = self_interaction & 3;
    int rc;
    if (bits == 8) rc = idx_bits == 64 ? launch_quant_nb<8, long long>(qa, x, x_ld, B, F, self, R, ldr, st)
                                       : launch_quant_nb<8, int>(qa, x, x_ld, B, F, self, R, ldr, st);
    else           rc = idx_bits == 64 ? launch_quant_nb<4, long long>(qa, x, x_ld, B, F, self, R, ldr, st)
                                       : launch_quant_nb<4, int>(qa, x, x_ld, B, F, self, R, ldr, st);
    if (rc) return rc;
    DLRM_LAUNCH_CHECK();
    return 0;
}
