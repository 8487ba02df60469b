// Eval-mode TRU-Net forward as ONE launch on the int8 MFMA (v_mfma_i32_16x16x64_i8): the quantized artefact of
// tinyrecurrentunet_amd/quantize.py.  The frame flow and the vector-ALU layers are those of
// stream_fwd.hip (section 3a), the LDS regions and helpers shared with it (stream_common.hpp); what differs is every matrix layer:
//
//   weights   int8, symmetric, one fp32 scale per output row of the folded matrix, 16-row tiles in fragment order
//             ([K/64 quads: lane l holds A[row l & 15][k = 64 ks + 16 (l >> 4) + 0..15]][16 scales][16 biases]);
//   operand   quantized per frame and per layer: ONE scale over the whole K x P operand (amax = max |x|, inv = 127 / amax,
//             q = clamp(rne(x inv), -127, 127)), written as a position-major int8 image [position][K + 16 bytes] so that a
//             lane's 16 consecutive K values of one column are one ds_read_b128;
//   result    exact int32 accumulation, z = float(acc) * (s_w[row] * s_x) + bias[row] in fp32, s_x = amax / 127.
//
// The fp32 arena already takes all 160 KiB, so the image is written IN PLACE: a pass reads the whole operand into registers
// (at most 96 values per thread), reduces |x| to the frame's amax (wave max + one LDS word per wave, one barrier), and only
// then writes the image over the region it was read from (the layer's output goes to another region, as in the fp32 kernel).
// The GRU recurrence weights W_hh are int8 with per-row scales too, dequantized once into the registers the fp32 kernel
// pins them in; the recurrence, the first conv, the depthwise convs and the last 8 -> 8 transposed conv stay fp32.
#include "stream_common.hpp"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int SI_RED = SF_R2 + 3584;     // the quantizer's per-wave amax (behind stream_common.hpp's GRU state)
constexpr int SI_NOFF = 26;
constexpr int SI_PAD = 512;              // words behind the last section: the 3-tap ConvT tiles are requested as 5 quads

// words of one 16-row tile with KS quads of A fragments: the quads, then 16 fp32 row scales and 16 fp32 biases
__host__ __device__ constexpr long long si_tile(int ks) { return 256LL * ks + 32; }

// Section bounds of the int8 image (offsets in 32-bit words): run by the host entry points AND again by the kernel.
__host__ __device__ inline int si_check(const int32_t* o, int n, long long words, int Cin) {
    if (!o || n != SI_NOFF || (Cin != 3 && Cin != 4) || words <= 0) return TRUNET_EINVAL;
    long long size[SI_NOFF];
    int i = 0;
    size[i++] = 64 * Cin * 5 + 64;                                     // first conv (fp32)
    size[i++] = 8 * si_tile(1);                                        // encoder.1 pw 128 x 64
    for (int k = 0; k < 4; ++k) size[i++] = 8 * si_tile(2);            // encoder.2..5 pw 128 x 128
    for (int k = 0; k < 5; ++k) size[i++] = 128 * (k & 1 ? 5 : 3) + 128;   // depthwise (fp32)
    size[i++] = 24 * si_tile(2);                                       // FGRU input projection 384 x 128
    size[i++] = 2 * 6 * 128 * 4 + 4 * 192;                             // W_hh int8 [2][6][128][16 B], scales, b_hh
    size[i++] = 4 * si_tile(2);                                        // FGRU.conv 64 x 128
    size[i++] = 4 * si_tile(1);                                        // decoder.0 pw 64 x 64
    for (int k = 0; k < 4; ++k) size[i++] = 4 * si_tile(3);            // decoder.1..4 pw 64 x 192
    size[i++] = si_tile(2);                                            // decoder.5 pw 8 (16) x 128
    for (int k = 0; k < 5; ++k) size[i++] = 4 * si_tile(k & 1 ? 5 : 3);   // transposed convs 64 x taps * 64
    size[i++] = 8 * 8 * 5 + 8;                                         // last ConvT (fp32)
    for (int k = 0; k < SI_NOFF; ++k) {
        const long long a = o[k];
        if (a < 0 || (a & 3)) return TRUNET_EINVAL;
        if (a + size[k] + SI_PAD > words) return TRUNET_EINVAL;
    }
    return TRUNET_OK;
}

// bare `ds_read_b128 v, base offset:imm` for the B operand: the lane's base is opaque, the stream's offsets immediates
typedef __attribute__((address_space(3))) const i32x4* si_lptr;
__device__ __forceinline__ si_lptr si_lds_base(const char* p) {
    si_lptr q = (si_lptr)p;
    asm volatile("" : "+v"(q));
    return q;
}

// ---- fragments of the wave's row tiles: NQ quads of A (fixed request size), row scales and biases of the lane's 4 rows
template <int NQ>
__device__ __forceinline__ void si_load(i32x4* fa, f32x4& sw, f32x4& bb, const uint32_t* tile, int ks, int lane) {
    const i32x4* p = (const i32x4*)tile + lane;
#pragma unroll
    for (int i = 0; i < NQ; ++i) fa[i] = p[i * 64];
    const f32x4* s = (const f32x4*)(tile + 256 * ks) + (lane >> 4);
    sw = s[0];
    bb = s[4];
}

// ---- the activation quantizer.  Operand rows k < K1 come from src1 (row stride ls1, column offset c1: the crops of the
// decoder's skip concatenation), rows k >= K1 from src2 (ls2); image position i is column i - G of the source (G = 4: the
// zero guard columns of a transposed conv's input, read by its shifted taps).  The image at `img` (floats from the LDS
// base) is [NP][KST bytes], position-major.  Thread work item = (position, 4 consecutive k): consecutive lanes read
// consecutive columns of a row and write one 32-bit word.  All reads happen before the barrier, all writes after it: the
// image may overwrite the operand.  Returns the frame's amax (identical in every thread).
template <int NW>
__device__ __forceinline__ float si_quant(float* lds, int src1, int ls1, int c1, int K1, int src2, int ls2, int K, int NP,
                                          int G, int img, int KST) {
    const int t = sf_tid();
    const int KG = K >> 2, di = SF_T % NP, dg = SF_T / NP;
    float v[NW][4];
    float m = 0.f;
    {
        int i = t % NP, g = t / NP;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (g < KG) {
                const int k = 4 * g;
                const bool first = k < K1;
                const int ls = first ? ls1 : ls2;
                const float* p = lds + (first ? src1 + k * ls1 + c1 : src2 + (k - K1) * ls2) + 4 + i - G;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[w][e] = p[e * ls];
                    m = fmaxf(m, fabsf(v[w][e]));
                }
            }
            i += di; g += dg;
            if (i >= NP) { i -= NP; ++g; }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    if ((t & 63) == 0) lds[SI_RED + (t >> 6)] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(lds[SI_RED], lds[SI_RED + 1]), fmaxf(lds[SI_RED + 2], lds[SI_RED + 3]));
    const float inv = amax > 0.f ? 127.f / amax : 0.f;
    char* im = (char*)(lds + img);
    {
        int i = t % NP, g = t / NP;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (g < KG) {
                uint32_t word = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float q = fminf(fmaxf(__builtin_rintf(v[w][e] * inv), -127.f), 127.f);
                    word |= ((uint32_t)(int)q & 255u) << (8 * e);
                }
                *(uint32_t*)(im + i * KST + 4 * g) = word;
            }
            i += di; g += dg;
            if (i >= NP) { i -= NP; ++g; }
        }
    }
    __syncthreads();
    return amax;
}

// acc[ct] += A(af[0..KS)) * B for NCT column tiles of 16: S is the lane's byte address in the image (position of column
// l & 15 of the first tile, k = 16 (l >> 4)); column tile ct is 16 positions further, k-step ks 64 bytes further.
template <int KS, int NCT, int KST>
__device__ __forceinline__ void si_mm(i32x4 (&acc)[NCT], const i32x4* af, const char* S) {
    const si_lptr b0 = si_lds_base(S);
    i32x4 b[KS * NCT];
#pragma unroll
    for (int x = 0; x < KS * NCT; ++x) b[x] = b0[(x % NCT) * KST + 4 * (x / NCT)];
#pragma unroll
    for (int x = 0; x < KS * NCT; ++x)
        acc[x % NCT] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[x / NCT], b[x], acc[x % NCT], 0, 0, 0);
}

// Pointwise conv (+ folded BatchNorm) on the image: TPW row tiles per wave (tile rt0 + 4 t + wave, or tile 0 with SPLIT, the
// waves then splitting the column groups of 16 NCT), P output positions, M rows, result fp32 into dst [row][lsd].
template <int KS, int NCT, int TPW, bool SPLIT, bool RELU, bool FULL>
__device__ __forceinline__ void si_pw(const i32x4* fa, const f32x4* sw, const f32x4* bb, float amax, const float* lds_c,
                                      float* lds, int img, int dst, int lsd, int P, int M) {
    constexpr int KST = 64 * KS + 16;
    const int tid_ = sf_tid();
    const int lane = tid_ & 63, wave = __builtin_amdgcn_readfirstlane(tid_ >> 6), q = lane >> 4, j = lane & 15;
    const float sx = amax / 127.f;
    const int ng = (P + 16 * NCT - 1) / (16 * NCT);
    const char* im = (const char*)(lds_c + img) + j * KST + 16 * q;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int row = 16 * (SPLIT ? 0 : 4 * t + wave) + 4 * q;
        f32x4 sc;
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[r] = sw[t][r] * sx;
        for (int g = SPLIT ? wave : 0; g < ng; g += SPLIT ? 4 : 1) {
            i32x4 acc[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = i32x4{0, 0, 0, 0};
            const int c0 = g * 16 * NCT;
            si_mm<KS, NCT, KST>(acc, fa + KS * t, im + c0 * KST);
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int col = c0 + 16 * ct + j;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = (float)acc[ct][r] * sc[r] + bb[t][r];
                    if (RELU) v = fmaxf(v, 0.f);
                    if (FULL || (col < P && row + r < M)) lds[dst + (row + r) * lsd + 4 + col] = v;
                }
            }
        }
    }
}

// ConvTranspose1d(64 -> 64, k = TAPS, stride S_, padding S_/2) + folded BatchNorm + ReLU: one 16-row tile per wave, per tap
// a dense GEMM over the parity class e of the output positions p = S_ j + e (as sf_convT16 of stream_fwd.hip); the image
// holds the input with G = 4 guard positions on each side.  Only [p0, p0 + Ln) is produced.
template <int TAPS, int S_, int NCT, bool FULL>
__device__ __forceinline__ void si_convT(const i32x4* fa, f32x4 sw, f32x4 bb, float amax, float* lds, int img, int dst,
                                         int lsd, int Lout, int p0, int Ln) {
    constexpr int KST = 80, PAD = S_ / 2;
    const int tid_ = sf_tid();
    const int lane = tid_ & 63, wave = __builtin_amdgcn_readfirstlane(tid_ >> 6), q = lane >> 4, j = lane & 15;
    const int pend = min(Lout, p0 + Ln);
    const int row = 16 * wave + 4 * q;
    const float sx = amax / 127.f;
    f32x4 sc;
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = sw[r] * sx;
    const char* im = (const char*)(lds + img) + (j + 4) * KST + 16 * q;
#pragma unroll
    for (int e = 0; e < S_; ++e) {
        const int j0 = p0 > e ? (p0 - e + S_ - 1) / S_ : 0;
        const int nj = (pend - e + S_ - 1) / S_ - j0;
        const int ng = (nj + 16 * NCT - 1) / (16 * NCT);
        for (int g = 0; g < ng; ++g) {
            i32x4 acc[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) acc[ct] = i32x4{0, 0, 0, 0};
            const int c0 = j0 + g * 16 * NCT;
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                constexpr int BIG = 8 * S_;
                if ((e + PAD - tap + BIG) % S_ == 0) {
                    const int d = (e + PAD - tap + BIG) / S_ - 8;
                    si_mm<1, NCT, KST>(acc, fa + tap, im + (c0 + d) * KST);
                }
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const int p = S_ * (c0 + 16 * ct + j) + e;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = fmaxf((float)acc[ct][r] * sc[r] + bb[r], 0.f);
                    if (FULL || p < pend) lds[dst + (row + r) * lsd + 4 + p] = v;
                }
            }
        }
    }
}

struct SiArgs {
    const float* x; float* y; const uint32_t* blob; float* scratch;
    long long words;
    int N, Cin;
    int o[SI_NOFF];        // first | pw[5] | dw[5] | gi | whh | fg | dpw[6] | ct[5] | last
};
enum { O_FIRST = 0, O_PW = 1, O_DW = 6, O_GI = 11, O_WHH = 12, O_FG = 13, O_DPW = 14, O_CT = 20, O_LAST = 25 };

#define SI_SYNC() __syncthreads()

__global__ __launch_bounds__(SF_T, 1) void stream_fwd_i8_kernel(const SiArgs A) {
    // the device's own bounds check of the section table (uniform: every thread returns before touching memory)
    if (si_check(A.o, SI_NOFF, A.words, A.Cin) != TRUNET_OK) return;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* skip = A.scratch + (size_t)blockIdx.x * SF_SKIP;
    float* sk0 = skip, *sk1 = sk0 + 8192, *sk2 = sk1 + 16384, *sk3 = sk2 + 8192, *sk4 = sk3 + 8192;
    const int Cin = A.Cin;
    const float* blobf0 = (const float*)A.blob;

    for (int i = tid; i < 64 * Cin * 5 + 64; i += SF_T) lds[SF_W0 + i] = blobf0[A.o[O_FIRST] + i];
    float xr[5];
    auto request_x = [&](int nn) __attribute__((always_inline)) {
        constexpr int LSX = sf_ls(257);
        const float* xg = A.x + (size_t)nn * Cin * 257;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int i = tid + SF_T * j;
            const int ch = i / LSX, col = i - ch * LSX - 4;
            xr[j] = (nn < A.N && ch < Cin && col >= 0 && col < 257) ? xg[ch * 257 + col] : 0.f;
        }
    };
    request_x(blockIdx.x);
    for (int n = blockIdx.x; n < A.N; n += gridDim.x) {
        // opaque per-frame offset of the blob: no fragment load is hoisted out of the frame loop (section 3a (1))
        int opaque0 = 0;
        asm volatile("" : "+s"(opaque0));
        const uint32_t* blob = A.blob + opaque0;
        const float* blobf = (const float*)blob;
        i32x4 fa[12];                    // A fragments of the wave's row tiles (at most 6 tiles x 2 quads)
        f32x4 sw[6], bb[6];              // their row scales and biases (the lane's 4 rows per tile)
        // ---------------- features -> LDS, first conv (C_in -> 64, k5 s2 p1) + ReLU (fp32)     network.py:9-21
        {
            constexpr int LSX = sf_ls(257);
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const int i = tid + SF_T * j;
                if (i < Cin * LSX) lds[SF_XB + i] = xr[j];
            }
            SI_SYNC();
            const int t_ = sf_tid();
            const int lo = t_ & 127, cg = __builtin_amdgcn_readfirstlane(t_ >> 7);
            float xin[4][5];
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    xin[ci][k] = ci < Cin ? lds[SF_XB + ci * LSX + 4 + 2 * lo - 1 + k] : 0.f;
            for (int co = 32 * cg; co < 32 * cg + 32; co += 4) {
                float v[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) v[jj] = lds[SF_W0 + 64 * Cin * 5 + co + jj];
#pragma unroll
                for (int ci = 0; ci < 4; ++ci) {
                    if (ci < Cin) {
#pragma unroll
                        for (int k = 0; k < 5; ++k)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj)
                                v[jj] = fmaf(lds[SF_W0 + (co + jj) * Cin * 5 + ci * 5 + k], xin[ci][k], v[jj]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) lds[SF_R0 + (co + jj) * LSA + 4 + lo] = fmaxf(v[jj], 0.f);
            }
            sf_guards(lds, SF_R0, 64, LSA, 128);
            SI_SYNC();
            sf_save(lds, SF_R0, LSA, sk0, 64, 5);
        }
        // ---------------- encoder.1: pw 64 -> 128 (int8), dw k3 s1                              network.py:24-43
        {
            float dwr[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) dwr[j] = blobf[A.o[O_DW] + tid + SF_T * j];
#pragma unroll
            for (int t = 0; t < 2; ++t) si_load<1>(fa + t, sw[t], bb[t], blob + A.o[O_PW] + (4 * t + wave) * si_tile(1), 1, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<8>(lds, SF_R0, LSA, 0, 64, 0, 0, 64, 128, 0, SF_R0, 80);
            si_pw<1, 2, 2, false, true, true>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1A, LSA, 128, 128);
            sf_guards(lds, SF_R1A, 128, LSA, 128);
#pragma unroll
            for (int j = 0; j < 2; ++j) lds[SF_DWB + tid + SF_T * j] = dwr[j];
            SI_SYNC();
            sf_dw<3, 1>(lds, SF_R1A, LSA, SF_R0, LSA, SF_DWB, 128, 128);
            sf_guards(lds, SF_R0, 128, LSA, 128);
            SI_SYNC();
            sf_save(lds, SF_R0, LSA, sk1, 128, 5);
        }
        // ---------------- encoder.2 .. encoder.5: ONE loop body (same load sequence every iteration)
        for (int it = 0; it < 4; ++it) {
            const int L = it == 0 ? 128 : (it <= 2 ? 64 : 32);
            float dwr[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) dwr[j] = blobf[A.o[O_DW + 1 + it] + tid + SF_T * j];
#pragma unroll
            for (int t = 0; t < 2; ++t)
                si_load<2>(fa + 2 * t, sw[t], bb[t], blob + A.o[O_PW + 1 + it] + (4 * t + wave) * si_tile(2), 2, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<16>(lds, SF_R0, LSA, 0, 128, 0, 0, 128, L, 0, SF_R0, 144);
            si_pw<2, 2, 2, false, true, true>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1A, LSA, L, 128);
            sf_guards(lds, SF_R1A, 128, LSA, L);
#pragma unroll
            for (int j = 0; j < 3; ++j) lds[SF_DWB + tid + SF_T * j] = dwr[j];
            SI_SYNC();
            if (it == 1) sf_dw<3, 1>(lds, SF_R1A, LSA, SF_R0, LSA, SF_DWB, 128, 64);
            else if (it == 3) sf_dw<3, 2>(lds, SF_R1A, LSA, SF_R0, LSA, SF_DWB, 128, 16);
            else sf_dw<5, 2>(lds, SF_R1A, LSA, SF_R0, LSA, SF_DWB, 128, L >> 1);
            const int Lo = it == 1 ? 64 : (L >> 1);
            sf_guards(lds, SF_R0, 128, LSA, Lo);
            SI_SYNC();
            if (it < 3) sf_save(lds, SF_R0, LSA, it == 0 ? sk2 : (it == 1 ? sk3 : sk4), 128, it == 2 ? 3 : 4);
        }
        // ---------------- FGRU input projection (384 x 128, both directions) over 16 positions: 6 row tiles per wave
#pragma unroll
        for (int t = 0; t < 6; ++t) si_load<2>(fa + 2 * t, sw[t], bb[t], blob + A.o[O_GI] + (4 * t + wave) * si_tile(2), 2, lane);
        __builtin_amdgcn_sched_barrier(0);
        {
            const float am = si_quant<2>(lds, SF_R0, LSA, 0, 128, 0, 0, 128, 16, 0, SF_R0, 144);
            si_pw<2, 1, 6, false, false, true>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1A, LSG, 16, 384);
        }
        SI_SYNC();
        {
            // recurrence (fp32, as stream_fwd.hip): direction d = tid >> 7; hidden unit j owned by the lane pair (2 j, 2 j + 1),
            // lane half kh holds the K-half [32 kh, 32 kh + 32) of the unit's r, z, n rows of W_hh -- int8 in the image
            // ([direction][6 quads: gate g, 16-column half h][128 threads][16 bytes], then scales [2][192], b_hh [2][192]),
            // dequantized once into the registers the recurrence keeps them in
            const int t_ = sf_tid();
            const int d = t_ >> 7, j = (t_ & 127) >> 1, kh = t_ & 1;
            const i32x4* whq = (const i32x4*)(blob + A.o[O_WHH]) + (size_t)d * 6 * 128 + (t_ & 127);
            const float* wsc = blobf + A.o[O_WHH] + 2 * 6 * 128 * 4 + d * 192;
            const float* bhh = wsc + 2 * 192;
            const float s3[3] = {wsc[j], wsc[64 + j], wsc[128 + j]};
            float w3[3][32];
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const i32x4 qv = whq[(2 * g + h) * 128];
#pragma unroll
                    for (int w = 0; w < 4; ++w)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            w3[g][16 * h + 4 * w + b] = (float)(int)(signed char)(qv[w] >> (8 * b)) * s3[g];
                }
            float* wr = w3[0], *wz = w3[1], *wn = w3[2];
#pragma unroll
            for (int k = 0; k < 32; ++k) asm volatile("" : "+v"(wr[k]), "+v"(wz[k]), "+v"(wn[k]));
            const float br = bhh[j], bz = bhh[64 + j], bn = bhh[128 + j];
            float* hs = lds + SF_GRU + d * 128;
            if ((t_ & 127) < 64) hs[t_ & 127] = 0.f;
            float hme = 0.f;
            SI_SYNC();
            for (int st = 0; st < 16; ++st) {
                const int pos = d ? 15 - st : st;
                const float* hc = hs + (st & 1) * 64 + 32 * kh;
                const float* gi = lds + SF_R1A + (d * 192 + j) * LSG + 4 + pos;
                const float gir = gi[0], giz = gi[64 * LSG], gin = gi[128 * LSG];
                f32x4 hv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) hv[i] = *(const f32x4*)(hc + 4 * i);
                float r0 = 0.f, r1 = 0.f, z0 = 0.f, z1 = 0.f, n0_ = 0.f, n1 = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    r0 = fmaf(wr[4 * i], hv[i][0], r0); r1 = fmaf(wr[4 * i + 1], hv[i][1], r1);
                    r0 = fmaf(wr[4 * i + 2], hv[i][2], r0); r1 = fmaf(wr[4 * i + 3], hv[i][3], r1);
                    z0 = fmaf(wz[4 * i], hv[i][0], z0); z1 = fmaf(wz[4 * i + 1], hv[i][1], z1);
                    z0 = fmaf(wz[4 * i + 2], hv[i][2], z0); z1 = fmaf(wz[4 * i + 3], hv[i][3], z1);
                    n0_ = fmaf(wn[4 * i], hv[i][0], n0_); n1 = fmaf(wn[4 * i + 1], hv[i][1], n1);
                    n0_ = fmaf(wn[4 * i + 2], hv[i][2], n0_); n1 = fmaf(wn[4 * i + 3], hv[i][3], n1);
                }
                float gr = r0 + r1, gz = z0 + z1, gn = n0_ + n1;
                gr += sf_dpp_xor1(gr); gz += sf_dpp_xor1(gz); gn += sf_dpp_xor1(gn);
                const float r = sf_sigmoid(gir + gr + br);
                const float z = sf_sigmoid(giz + gz + bz);
                const float nn = sf_tanh(fmaf(r, gn + bn, gin));
                hme = (1.f - z) * nn + z * hme;
                if (kh == 0) {
                    hs[((st + 1) & 1) * 64 + j] = hme;
                    lds[SF_R0 + (d * 64 + j) * LSA + 4 + pos] = hme;
                }
                SI_SYNC();
            }
            sf_guards(lds, SF_R0, 128, LSA, 16);
            SI_SYNC();
        }
        // ---------------- FGRU.conv (128 -> 64) + BN + ReLU
        {
            si_load<2>(fa, sw[0], bb[0], blob + A.o[O_FG] + wave * si_tile(2), 2, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<2>(lds, SF_R0, LSA, 0, 128, 0, 0, 128, 16, 0, SF_R0, 144);
            si_pw<2, 1, 1, false, true, true>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1A, LSA, 16, 64);
            sf_guards(lds, SF_R1A, 64, LSA, 16);
            SI_SYNC();
        }
        // ---------------- decoder.0 (FirstTrCNN): pw 64 -> 64, ConvT k3 s2 -> L 31            network.py:60-76
        {
            si_load<1>(fa, sw[0], bb[0], blob + A.o[O_DPW] + wave * si_tile(1), 1, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<1>(lds, SF_R1A, LSA, 0, 64, 0, 0, 64, 16, 0, SF_R1A, 80);
            si_pw<1, 1, 1, false, true, true>(fa, sw, bb, am, lds, lds, SF_R1A, SF_R1B, LSA, 16, 64);
            sf_guards(lds, SF_R1B, 64, LSA, 16);
            SI_SYNC();
            sf_restore(lds, SF_R0, LSA, sk4, 128, 3);
            si_load<3>(fa, sw[0], bb[0], blob + A.o[O_CT] + wave * si_tile(3), 3, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am2 = si_quant<2>(lds, SF_R1B, LSA, 0, 64, 0, 0, 64, 24, 4, SF_R1B, 80);
            si_convT<3, 2, 1, false>(fa, sw[0], bb[0], am2, lds, SF_R1B, SF_R1A, LSA, 31, 0, 31);
            sf_guards(lds, SF_R1A, 64, LSA, 31);
            SI_SYNC();
        }
        // ---------------- decoder.1 .. decoder.4 (TrCNN): [x1 padded / cropped | skip] -> pw 192 -> 64 -> ConvT
        // (stream_fwd.hip's loop: the next block's skip tensor is requested a block ahead and written to R0 after the ConvT)
        for (int i = 1; i <= 4; ++i) {
            const int P = i == 1 ? 32 : (i == 4 ? 128 : 64);
            const int Lo = i == 1 ? 65 : (i == 2 ? 66 : (i == 3 ? 129 : 130));
            si_load<3>(fa, sw[0], bb[0], blob + A.o[O_DPW + i] + wave * si_tile(3), 3, lane);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 rr[16];
            const float* skn = i == 1 ? sk3 : (i == 2 ? sk2 : (i == 3 ? sk1 : sk0));
            const int skC = i == 4 ? 64 : 128, sklq = i <= 2 ? 4 : 5;
            sf_restore_request(rr, skn, skC, sklq);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<24>(lds, SF_R1A, LSA, i == 1 ? 0 : 1, 64, SF_R0, LSA, 192, P, 0, SF_R0, 208);
            si_pw<3, 2, 1, false, true, true>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1B, LSA, P, 64);
            sf_guards(lds, SF_R1B, 64, LSA, P);
            SI_SYNC();
            // ConvT fragments: 5 quads requested for the 3-tap layers too (same load sequence); scales behind the taps
            const int taps = (i & 1) ? 5 : 3;
            si_load<5>(fa, sw[0], bb[0], blob + A.o[O_CT + i] + wave * (256 * taps + 32), taps, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am2 = si_quant<9>(lds, SF_R1B, LSA, 0, 64, 0, 0, 64, P + 8, 4, SF_R1B, 80);
            const int Pn = i <= 2 ? 64 : 128;
            if (i & 1) si_convT<5, 2, 2, true>(fa, sw[0], bb[0], am2, lds, SF_R1B, SF_R1A, LSA, Lo, 1, Pn);
            else si_convT<3, 1, 2, true>(fa, sw[0], bb[0], am2, lds, SF_R1B, SF_R1A, LSA, Lo, 1, Pn);
            sf_restore_commit(rr, lds, SF_R0, LSA, skC, sklq);
            sf_guards(lds, SF_R1A, 64, LSA, Lo);
            SI_SYNC();
        }
        {   // ---------------- decoder.5 (LastTrCNN): pw 128 -> 8 (+BN+ReLU, int8), ConvT 8 -> 8 k5 s2 -> 257 (fp32), linear
            si_load<2>(fa, sw[0], bb[0], blob + A.o[O_DPW + 5], 2, lane);
            __builtin_amdgcn_sched_barrier(0);
            const float am = si_quant<16>(lds, SF_R1A, LSA, 1, 64, SF_R0, LSA, 128, 128, 0, SF_R0, 144);
            si_pw<2, 2, 1, true, true, false>(fa, sw, bb, am, lds, lds, SF_R0, SF_R1B, LSA, 128, 8);
            sf_guards(lds, SF_R1B, 8, LSA, 128);
            for (int i = tid; i < 8 * 8 * 5 + 8; i += SF_T) {
                int d = i;
                if (i < 320) {
                    const int ci = i / 40, r = i - ci * 40, co = r / 5, k = r - co * 5;
                    d = (((co >> 2) * 8 + ci) * 5 + k) * 4 + (co & 3);
                }
                lds[SF_DWB + d] = blobf[A.o[O_LAST] + i];
            }
            request_x(n + gridDim.x);
            SI_SYNC();
            float* yg = A.y + (size_t)n * 8 * 257;
            {
                const int t_ = sf_tid();
                const int j = t_ & 127, cg = __builtin_amdgcn_readfirstlane(t_ >> 7);
                const float* in = lds + SF_R1B + 4 + j;
                const f32x4* W4 = (const f32x4*)(lds + SF_DWB) + cg * 40;
                f32x4 a0 = *(const f32x4*)(lds + SF_DWB + 320 + 4 * cg), a1 = a0;
#pragma unroll
                for (int ci = 0; ci < 8; ++ci) {
                    const float xm = in[ci * LSA - 1], x0 = in[ci * LSA], xp = in[ci * LSA + 1];
                    const f32x4 w0 = W4[ci * 5], w1 = W4[ci * 5 + 1], w2 = W4[ci * 5 + 2], w3 = W4[ci * 5 + 3],
                                w4 = W4[ci * 5 + 4];
                    a0 += w1 * x0 + w3 * xm;
                    a1 += w0 * xp + w2 * x0 + w4 * xm;
                }
                float* yb = yg + (size_t)(4 * cg) * 257 + 2 * j;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) { yb[c4 * 257] = a0[c4]; yb[c4 * 257 + 1] = a1[c4]; }
                if (t_ < 8) {
                    float v = lds[SF_DWB + 320 + t_];
#pragma unroll
                    for (int ci = 0; ci < 8; ++ci)
                        v = fmaf(lds[SF_DWB + (((t_ >> 2) * 8 + ci) * 5 + 3) * 4 + (t_ & 3)], lds[SF_R1B + ci * LSA + 4 + 127], v);
                    yg[t_ * 257 + 256] = v;
                }
            }
            SI_SYNC();
        }
    }
}

// Lane maps of v_mfma_i32_16x16x64_i8 as this file uses them: A (16 x 64, row-major) in the exporter's fragment order, B
// (64 x 16, row-major) as the image reads give it, C (16 x 16) from the accumulator layout.  One wave.
__global__ void si_probe_kernel(const int8_t* Am, const int8_t* Bm, int* Cm) {
    const int l = threadIdx.x, q = l >> 4, j = l & 15;
    i32x4 a, b;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t wa = 0, wb = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            wa |= (uint32_t)(uint8_t)Am[j * 64 + 16 * q + 4 * w + e] << (8 * e);
            wb |= (uint32_t)(uint8_t)Bm[(16 * q + 4 * w + e) * 16 + j] << (8 * e);
        }
        a[w] = (int)wa;
        b[w] = (int)wb;
    }
    i32x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Cm[(4 * q + r) * 16 + j] = acc[r];
}

}  // namespace

extern "C" int trunet_stream_fwd_i8_check(const int32_t* h_offsets, int n_offsets, int64_t blob_bytes, int Cin) {
    if (blob_bytes <= 0 || (blob_bytes & 3)) return TRUNET_EINVAL;
    return si_check(h_offsets, n_offsets, blob_bytes >> 2, Cin);
}

extern "C" int trunet_stream_fwd_i8(const float* x, float* y, const void* blob, const int32_t* h_offsets, int n_offsets,
                                    int64_t blob_bytes, float* scratch, int N, int Cin, void* stream) {
    if (!x || !y || !blob || !h_offsets || !scratch || N <= 0) return TRUNET_EINVAL;
    if (Cin != 3 && Cin != 4) return TRUNET_ENOTSUP;
    {
        const int rc = trunet_stream_fwd_i8_check(h_offsets, n_offsets, blob_bytes, Cin);
        if (rc != TRUNET_OK) return rc;
    }
    SiArgs a;
    a.x = x; a.y = y; a.blob = (const uint32_t*)blob; a.scratch = scratch; a.words = blob_bytes >> 2; a.N = N; a.Cin = Cin;
    for (int k = 0; k < SI_NOFF; ++k) a.o[k] = h_offsets[k];
    const int grid = trunet_stream_fwd_grid(N);
    const size_t ldsb = (size_t)SF_ARENA * sizeof(float);
    if (hipFuncSetAttribute((const void*)stream_fwd_i8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(stream_fwd_i8_kernel, dim3(grid), dim3(SF_T), ldsb, (hipStream_t)stream, a);
    return trunet_launch_status();
}

extern "C" int trunet_i8_mfma_probe(const void* a, const void* b, int* c, void* stream) {
    if (!a || !b || !c) return TRUNET_EINVAL;
    hipLaunchKernelGGL(si_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int8_t*)a, (const int8_t*)b, c);
    return trunet_launch_status();
}
