// Fused backward of a ConvTranspose1d(64 -> 64, k = K, stride S, padding S/2) + BatchNorm layer (autograd of the reference's
// network.py:67,86 with the BatchNorm of :72,91 behind it and the BatchNorm+ReLU of :65-66,84-85 in front):
//   z[co][p][n] = b[co] + sum_{ci,k} W[ci][co][k] a[ci][q][n],  p = q S - pad + k,   a = max(sc zs + sh, 0)
// ONE pass over (dy, z, zs) produces
//   dz        = ca dy + cb z + cc                                   (BatchNorm backward of z: in LDS only)
//   dW, db    = sum_{q,n} a[ci][q] dz[co][q S - pad + k] ,  sum_{p,n} dz          (per-workgroup partial images)
//   g         = [sc zs + sh > 0] sum_{co,k} W[ci][co][k] dz[co][q S - pad + k]   -> gradient at the source's BatchNorm output
//   stats     = sum g, sum g (zs - mean)                            (BatchNorm backward of the source)
// The separate launches it replaces (conv_gemm data gradient over K tap segments + conv_wgrad over K tap segments) each
// read dy and z (the data gradient reads every dz row K/S times as a tap of different positions) and the source twice.
//
// Decomposition: a tile is (source position q, 32 frames).  A workgroup owns whole frame chunks and walks q = 0 .. Lin-1,
// so the dz rows p = q S - pad .. q S - pad + K - 1 form a sliding window: every dz row is loaded and BatchNorm-transformed
// ONCE per chunk into a ring of K + LA S row sets and serves all K taps (positions) that need it; every step brings S new dz
// rows (dy into the ring, z into a staging slot, combined in place by the thread that requested the piece) and one source
// row set.  LDS-DMA (global_load_lds) LA steps ahead (CtLds::LA: two, one in the stride-2 split instances), counted vmcnt,
// one barrier per step, 16-byte pieces XOR-swizzled through the source address as in conv_wgrad_kernel / pw_bwd_kernel.
//
// All 8 waves carry the same MFMA load (16 K per step, two waves per SIMD):
//   waves 0-3  loaders + weight gradient: wave (ci tile, co tile) keeps its K accumulators (one per tap) for the whole
//              kernel; the frame axis is the MFMA K axis; BatchNorm+ReLU of the source is applied to the A fragment on the fly
//   waves 4-7  data gradient: wave (ci tile, co half) keeps W^T fragments of its 32 co rows for all taps in registers;
//              the two co halves of a ci tile are combined through LDS, and the co-half-0 wave runs the epilogue (ReLU mask,
//              store, statistics) from registers after the barrier, in the shadow of the next step.
//
// ONE kernel source, two operand paths (template parameter X3).  X3 = false runs both GEMMs on the fp32 MFMA
// (v_mfma_f32_32x32x2_f32, two workgroups per CU).  X3 = true, the default of the training step (trunet_gemm_x3_enable /
// TRUNET_GEMM_X3, gemm_x3.hip), runs them on the bf16 MFMA through the three-term operand split of x3_common.hpp (round 4;
// fp32-grade result, one workgroup per CU).  Decomposition, rings, DMA schedule, prologue arithmetic and epilogue are the
// same text; what differs is how a staged fp32 fragment reaches the matrix pipe:
//   weight gradient (waves 0-3): per 16 frames the source row's 8 values of a lane (two swizzled 16-byte pieces) get
//       BatchNorm+ReLU and are split ONCE, every valid tap's dz row fragment comes as planes, 6 v_mfma_f32_32x32x16_bf16 per tap;
//   data gradient (waves 4-7): W^T of the wave's (ci tile, co half) for all taps sits in registers as three bf16 fragment
//       planes (split once per kernel), per tap and 16 co rows the lane's dz planes come through transposing reads, 6 MFMAs.
// Here a staged fragment feeds ONE 32-row tile per wave, so a split by the consuming wave is not amortised (about 7 vector
// instructions per MFMA: such waves are vector-bound; still well ahead of the fp32 MFMA, 6 x 33 matrix cycles + ~45 x 4
// vector cycles per (32 x 32 x 16) against 8 x 64) -- hence the dz planes below.  The fp32-MFMA instance was the most
// matrix-bound kernel of the step (matrix pipe 62-65 % busy, HBM at 0.25 of its peak).
#include <type_traits>
#include "dma_common.hpp"
#include "x3_common.hpp"

namespace {

constexpr int CT_F = 32;            // frames per tile
constexpr int CT_C = 64;            // channels (both sides)
constexpr int CT_SET = CT_C * CT_F; // floats per row set (8 KB)
constexpr int CT_GRID = TRUNET_NUM_CU;
constexpr int CT_LO = CT_C * 16;    // floats per row set of the lo-plane ring (8 bytes per 4 frames)

// (X3; as in pw_bwd.hip) dz is split ONCE, by the prologue pass that computes it: the dz ring keeps [hi | mid] of a piece's
// 4 frames in the piece's own 16 bytes, a second ring of 4 KB slots the lo plane.  The weight-gradient B fragments
// (K = frames) are then 8-byte reads, the data-gradient B fragments (K = dz rows) transposing reads (ds_read_b64_tr_b16),
// neither with vector work; only the source rows are still split by the wave that consumes them.  Needs RDZ x 4 KB more
// LDS.  With two steps of DMA lead (RDZ = K + 2 S, 2 S staging slots, 4 source slots) k3 s1 fits (126 KB); k3 s2 (166 KB)
// and k5 s2 (190 KB) do not, so the stride-2 split instances run with ONE step of lead (ct_lookahead): RDZ = K + S, S
// staging slots, 3 source slots -- k3 s2 118 KB, k5 s2 142 KB.  A step of k5 s2 lasts several microseconds: the rows of
// step q + 2 are requested behind the barrier that ends step q and awaited behind the last K-step of step q + 1.
template <int K, int S, bool X3>
constexpr int ct_lookahead() { return X3 && S == 2 ? 1 : 2; }

// float offset of the 8 lo bytes of logical piece `pc` of row `r` inside a lo-ring slot (same swizzle as the row set)
__device__ __forceinline__ int ct_lo_off(int r, int pc) { return r * 16 + 2 * (pc ^ ((r >> 1) & 7)); }

__device__ __forceinline__ void ct_bstore(__amdgpu_buffer_rsrc_t r, int voff, int soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}

// ring depths and the carve-up of the dynamic LDS (float offsets), for the kernel and its launcher
template <int K, int S, bool X3>
struct CtLds {
    static constexpr bool DZP = X3;
    static constexpr int LA = ct_lookahead<K, S, X3>();     // DMA lead in steps: behind the barrier of step q go the rows of step q + 1 + LA
    static_assert(LA == 1 || LA == 2, "the counted wait of the step loop leaves at most one issue in flight");
    static constexpr int RDZ = K + LA * S;      // dz ring: window + the rows of the next LA steps
    static constexpr int ZS = LA * S;           // z staging slots: the rows not yet transformed
    static constexpr int RS = LA + 2;           // source ring: q - 1 (its epilogue runs during step q), q .. q + LA
    static constexpr int DZ = 0;                                // [RDZ][64][32]
    static constexpr int ZST = DZ + RDZ * CT_SET;               // [ZS][64][32]
    static constexpr int SRC = ZST + ZS * CT_SET;               // [RS][64][32]
    static constexpr int PART = SRC + RS * CT_SET;              // [2 parity][2 ci tiles][16][64]
    static constexpr int LO = PART + 2 * 2 * 16 * 64;           // (DZP) [RDZ][64][16]: lo plane of the dz ring
    static constexpr int COEF = LO + (DZP ? RDZ * CT_LO : 0);   // f32x4 [2][64]: (ca, cb, cc, 0) of dz, (sc, sh, mean, 0) of the source
    static constexpr size_t BYTES = COEF * sizeof(float) + 2 * CT_C * sizeof(f32x4);
    static_assert(BYTES <= 160 * 1024, "LDS");
};

// W^T fragments of a data-gradient wave (row ci = 32 cit + c) for all taps, in the form its MFMA takes them
template <int K>
struct CtWtF32 { float af[K][16]; };                    // af[k][kk] = W[ci][co = 32 chf + 2 kk + h][k]
template <int K>
struct CtWtX3 { u32x4 A0[K][2], A1[K][2], A2[K][2]; };  // planes of co = 32 chf + 16 ks + 8 h + j, j < 8, per tap and K-step ks

template <int K, int S, bool X3>
__global__ __launch_bounds__(512, X3 ? 1 : 2) void convt_bwd_kernel(const trunet_convt_bwd_args a) {
    using L = CtLds<K, S, X3>;
    constexpr int PAD = S / 2, RDZ = L::RDZ, ZS = L::ZS, RS = L::RS, LA = L::LA;
    constexpr bool DZP = L::DZP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* DZ = smem + L::DZ;
    float* ZST = smem + L::ZST;
    float* SRC = smem + L::SRC;
    float* PART = smem + L::PART;
    float* LO = smem + L::LO;
    f32x4* CA = (f32x4*)(smem + L::COEF);
    f32x4* CB = CA + CT_C;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, c = lane & 31;
    const int NP = a.NP, Lin = a.Lin, Lout = a.Lout;

    for (int r = tid; r < CT_C; r += 512) {
        CA[r] = f32x4{a.ca[r], a.cb[r], a.cc[r], 0.f};
        CB[r] = f32x4{a.s_scale[r], a.s_shift[r], a.s_mean[r], 0.f};
    }
    // ring slot of dz row p for the fragment reads.  The stride-2 split instances pass it through an SGPR the compiler does
    // not see through: it otherwise folds the slot arithmetic into one lane address per (tap, read) -- about 40 VGPRs of
    // address constants in k5 s2, which then spills its W^T fragments
    auto dz_slot = [](int p) __attribute__((always_inline)) {
        if constexpr (X3 && S == 2) return wave_uniform(p % RDZ);
        else return p % RDZ;
    };
    const int nfc = NP / CT_F;
    const int c_begin = (int)(((long long)blockIdx.x * nfc) / gridDim.x);
    const int c_end = (int)(((long long)(blockIdx.x + 1) * nfc) / gridDim.x);
    __syncthreads();

    if (wave < 4) {
        // =============================================================== loaders + weight gradient
        const int cit = wave & 1, cot = wave >> 1;
        f32x16 acc[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
        float bsum[2] = {0.f, 0.f};
        const int pc = lane & 7;
        // this lane's rows in a row set: groups g = wave, wave + 4 -> row 8 g + (lane >> 3); logical piece folded in
        int row_[2], lc_[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            row_[i] = 8 * (wave + 4 * i) + (lane >> 3);
            lc_[i] = pc ^ ((row_[i] >> 1) & 7);
        }
        const float sc_a = a.s_scale[cit * 32 + c], sh_a = a.s_shift[cit * 32 + c];      // BN+ReLU of this lane's A row

        // DMA of dz rows [pa, pb) (dy -> ring slot p % RDZ, z -> staging slot p % ZS) and, with sq >= 0, of source row set
        // sq; returns the number of wave-instructions issued (rows outside [0, Lout) / [0, Lin) are skipped)
        auto issue = [&](int pa, int pb, int sq, int n0) __attribute__((always_inline)) -> int {
            int n = 0;
            for (int p = max(pa, 0); p < min(pb, Lout); ++p) {
                float* dst = DZ + (p % RDZ) * CT_SET;
                float* zst = ZST + (p % ZS) * CT_SET;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const size_t off = ((size_t)row_[i] * Lout + p) * NP + n0 + 4 * lc_[i];
                    __builtin_amdgcn_global_load_lds(a.dy + off, (lds_ptr_t)(dst + (wave + 4 * i) * 256), 16, 0, TRUNET_DMA_AUX);
                    __builtin_amdgcn_global_load_lds(a.z + off, (lds_ptr_t)(zst + (wave + 4 * i) * 256), 16, 0, TRUNET_DMA_AUX);
                }
                n += 4;
            }
            if (sq >= 0 && sq < Lin) {
                float* sdst = SRC + (sq % RS) * CT_SET;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const size_t off = ((size_t)row_[i] * Lin + sq) * NP + n0 + 4 * lc_[i];
                    __builtin_amdgcn_global_load_lds(a.src + off, (lds_ptr_t)(sdst + (wave + 4 * i) * 256), 16, 0, TRUNET_DMA_AUX);
                }
                n += 2;
            }
            return n;
        };
        // BatchNorm backward of dz rows [pa, pb) in place (this thread's own DMA pieces) + bias-gradient partial sums
        auto prologue = [&](int pa, int pb, int n0) __attribute__((always_inline)) {
            for (int p = max(pa, 0); p < min(pb, Lout); ++p) {
                float* dst = DZ + (p % RDZ) * CT_SET;
                const float* zst = ZST + (p % ZS) * CT_SET;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int o = row_[i] * CT_F + 4 * pc;
                    f32x4 v = *(f32x4*)(dst + o);
                    const f32x4 zz = *(const f32x4*)(zst + o);
                    const f32x4 k = CA[row_[i]];
                    float s = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = fmaf(k[0], v[e], fmaf(k[1], zz[e], k[2]));
                        if (n0 + 4 * lc_[i] + e >= a.N) v[e] = 0.f;
                        s += v[e];
                    }
                    bsum[i] += s;
                    if constexpr (DZP) {
                        unsigned h0, m0, l0, h1, m1, l1;
                        ctx_split2(v[0], v[1], h0, m0, l0);
                        ctx_split2(v[2], v[3], h1, m1, l1);
                        *(u32x4*)(dst + o) = u32x4{h0, h1, m0, m1};
                        *(u32x2*)(LO + (p % RDZ) * CT_LO + row_[i] * 16 + 2 * pc) = u32x2{l0, l1};
                    } else {
                        *(f32x4*)(dst + o) = v;
                    }
                }
            }
        };
        // dz rows first needed at step q >= 1: the S highest rows of its window
        auto new_lo = [&](int q) { return q * S - PAD + K - S; };

        // K-steps of a position (the fp32 MFMA takes 8 frames, the six bf16 MFMAs 16) and the one that carries the
        // prologue of the next position.  With one step of lead that is the last one: the rows were requested behind the
        // barrier that opened this step, and the wait in front of the prologue is the only place where the wave can stand
        // for them (k5 s2: 1.88 ms per step against 1.96 ms with the prologue behind the first K-step, profiles/ctb2_a)
        constexpr int NQQ = X3 ? CT_F / 16 : CT_F / 8, QQ_PRO = X3 ? (LA == 1 ? NQQ - 1 : 0) : 1;

        for (int ch = c_begin; ch < c_end; ++ch) {
            const int n0 = ch * CT_F;
            // ---- run start: the window of step 0 and the rows of the steps below LA, ZS rows at a time (the z staging area
            // holds ZS row sets), sources 0 .. LA - 1 (LA <= 2: source 1 rides with the second batch of rows, or alone when
            // there is none); then the rows of step LA go in flight
            {
                const int pa = -PAD, pb = new_lo(LA - 1) + S;       // rows of steps 0 .. LA - 1
                for (int p = pa; p < pb; p += ZS) {
                    issue(p, min(p + ZS, pb), p == pa ? 0 : (LA == 2 && p == pa + ZS ? 1 : -1), n0);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    prologue(p, min(p + ZS, pb), n0);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                if (LA == 2 && pb - pa <= ZS) { issue(0, 0, 1, n0); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
            }
            int n_last = issue(new_lo(LA), new_lo(LA) + S, LA, n0);     // rows of step LA (only when Lin > LA)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            for (int q = 0; q < Lin; ++q) {
                const float* Ssrc = SRC + (q % RS) * CT_SET;
                const int ra = cit * 32 + c, rb = cot * 32 + c;
#pragma unroll
                for (int qq = 0; qq < NQQ; ++qq) {
                    if constexpr (X3) {
                        // this lane's 8 frames of the K-step: 16 qq + 8 h .. + 7 = pieces 4 qq + 2 h, 4 qq + 2 h + 1 of its row
                        f32x4 av0 = *(const f32x4*)(Ssrc + swz_off(ra, 4 * qq + 2 * h));
                        f32x4 av1 = *(const f32x4*)(Ssrc + swz_off(ra, 4 * qq + 2 * h + 1));
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            av0[e] = fmaxf(fmaf(av0[e], sc_a, sh_a), 0.f);
                            av1[e] = fmaxf(fmaf(av1[e], sc_a, sh_a), 0.f);
                        }
                        u32x4 a0, a1, a2;
                        ctx_split8(av0, av1, a0, a1, a2);
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const int p = q * S - PAD + k;
                            if (p >= 0 && p < Lout) {
                                const int sl = dz_slot(p);
                                // the dz planes as the prologue left them: [hi | mid] in the piece, lo in the lo ring
                                const float* Dp = DZ + sl * CT_SET;
                                const float* Lp = LO + sl * CT_LO;
                                const u32x4 q0 = *(const u32x4*)(Dp + swz_off(rb, 4 * qq + 2 * h));
                                const u32x4 q1 = *(const u32x4*)(Dp + swz_off(rb, 4 * qq + 2 * h + 1));
                                const u32x2 l0 = *(const u32x2*)(Lp + ct_lo_off(rb, 4 * qq + 2 * h));
                                const u32x2 l1 = *(const u32x2*)(Lp + ct_lo_off(rb, 4 * qq + 2 * h + 1));
                                const u32x4 b0 = {q0[0], q0[1], q1[0], q1[1]}, b1 = {q0[2], q0[3], q1[2], q1[3]},
                                            b2 = {l0[0], l0[1], l1[0], l1[1]};
                                CTX_MF6(acc[k], a0, a1, a2, b0, b1, b2);
                            }
                        }
                    } else {
                        f32x4 av = *(const f32x4*)(Ssrc + swz_off(ra, 2 * qq + h));
#pragma unroll
                        for (int e = 0; e < 4; ++e) av[e] = fmaxf(fmaf(av[e], sc_a, sh_a), 0.f);
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const int p = q * S - PAD + k;
                            if (p >= 0 && p < Lout) {
                                const f32x4 bv = *(const f32x4*)(DZ + (p % RDZ) * CT_SET + swz_off(rb, 2 * qq + h));
#pragma unroll
                                for (int j = 0; j < 4; ++j)
                                    acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc[k], 0, 0, 0);
                            }
                        }
                    }
                    if (qq == QQ_PRO && q >= LA - 1) {
                        // outstanding: the rows of step q + 1 (oldest) and, with LA = 2, of step q + 2 (the newest n_last):
                        // transform the rows of step q + 1 in the shadow of this step's MFMAs
                        wait_vmcnt_exact<31>(LA == 2 ? n_last : 0);
                        prologue(new_lo(q + 1), new_lo(q + 1) + S, n0);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();            // every LDS read of step q is done; step q + 1 is staged
                asm volatile("" ::: "memory");
                // free now: the ring slots of the rows that left the window, S staging slots, source slot (q + 1 + LA) % RS
                n_last = (q + 1 + LA < Lin) ? issue(new_lo(q + 1 + LA), new_lo(q + 1 + LA) + S, q + 1 + LA, n0) : 0;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                // the rings are reused by the next chunk
            asm volatile("" ::: "memory");
        }
        // ---- this workgroup's partial image of dW (native ConvTranspose1d layout (Ci, Co, K)) and db
        float* img = a.w_partials + (size_t)blockIdx.x * a.w_numel;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = cit * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int co = cot * 32 + c;
                img[((size_t)ci * CT_C + co) * K + k] = acc[k][r];
            }
        if (a.b_partials) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float v = bsum[i];
                v += __shfl_xor(v, 4);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 1);
                if ((lane & 7) == 0) a.b_partials[(size_t)blockIdx.x * a.b_stride + a.b_off + row_[i]] = v;
            }
        }
    } else {
        // =============================================================== data gradient
        const int jj = wave - 4;
        const int cit = jj & 1, chf = jj >> 1;           // ci tile, co half
        const int trr = 8 * (lane >> 5) + ((lane & 15) >> 2), trp = 4 * ((lane >> 4) & 1) + (lane & 3);     // (DZP) transposing reads
        std::conditional_t<X3, CtWtX3<K>, CtWtF32<K>> wt;
        if constexpr (X3) {
            const float* wp = a.W + ((size_t)(cit * 32 + c) * CT_C + chf * 32 + 8 * h) * K;
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    f32x4 w0, w1;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w0[j] = wp[(size_t)(16 * ks + j) * K + k];
                        w1[j] = wp[(size_t)(16 * ks + 4 + j) * K + k];
                    }
                    ctx_split8(w0, w1, wt.A0[k][ks], wt.A1[k][ks], wt.A2[k][ks]);
                }
        } else {
            const float* wp = a.W + ((size_t)(cit * 32 + c) * CT_C + chf * 32 + h) * K;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
#pragma unroll
                for (int k = 0; k < K; ++k) wt.af[k][kk] = wp[(size_t)(2 * kk) * K + k];
        }
        float st1[16], st2[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { st1[r] = 0.f; st2[r] = 0.f; }
        const size_t dstride = (size_t)Lin * NP;
        const int rowb = (int)(dstride * sizeof(float));
        const int voff = (int)((4 * h * dstride + c) * sizeof(float));

        f32x16 dacc;
        auto epilogue = [&](int q, int n0) __attribute__((always_inline)) {
            // val = own half + the other co half (through LDS), ReLU mask from the raw source row set, store, statistics
            const float* P = PART + ((q & 1) * 2 + cit) * 16 * 64 + lane;
            const float* Ssrc = SRC + (q % RS) * CT_SET;
            const __amdgpu_buffer_rsrc_t ro = buffer_rsrc(a.dsrc + (size_t)(32 * cit) * dstride + (size_t)q * NP);
            const bool fin = n0 + c < a.N;
            const int nb = n0 * (int)sizeof(float);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (r & 3) + 8 * (r >> 2);
                const int row = cit * 32 + ml + 4 * h;
                const float zs = Ssrc[row * CT_F + 4 * ((c >> 2) ^ ((row >> 1) & 7)) + (c & 3)];
                const f32x4 k = CB[row];
                float val = dacc[r] + P[r * 64];
                val = (fmaf(k[0], zs, k[1]) > 0.f) ? val : 0.f;
                ct_bstore(ro, voff, ml * rowb + nb, val);
                const float x = fin ? val : 0.f;
                st1[r] += x;
                st2[r] = fmaf(x, zs - k[2], st2[r]);
            }
        };

        for (int ch = c_begin; ch < c_end; ++ch) {
            const int n0 = wave_uniform(ch * CT_F);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();                // step 0 staged
            asm volatile("" ::: "memory");
            for (int q = 0; q < Lin; ++q) {
#pragma unroll
                for (int r = 0; r < 16; ++r) dacc[r] = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int p = q * S - PAD + k;
                    if (p < 0 || p >= Lout) continue;
                    // B fragment: this lane's frame c of the dz rows of the wave's co half; row r keeps its 16-byte pieces
                    // XOR-swizzled by (r >> 1) & 7
                    if constexpr (DZP) {
                        // K-step ks: lane (G = lane >> 4, i = lane & 15) fetches the 4 frames of logical piece 4 (G & 1) + (i & 3) of row
                        // 32 chf + 16 ks + 8 h + 4 t + (i >> 2) and receives frame c of the rows 8 h + 4 t .. + 3 (t = 0, 1)
                        const int sl = dz_slot(p);
                        const float* Dq = DZ + sl * CT_SET;
                        const float* Lq = LO + sl * CT_LO;
#pragma unroll
                        for (int ks = 0; ks < 2; ++ks) {
                            const int r0 = chf * 32 + 16 * ks + trr;
                            const u32x2 h0 = lds_tr16(Dq + swz_off(r0, trp)), h1 = lds_tr16(Dq + swz_off(r0 + 4, trp));
                            const u32x2 m0 = lds_tr16(Dq + swz_off(r0, trp) + 2), m1 = lds_tr16(Dq + swz_off(r0 + 4, trp) + 2);
                            const u32x2 l0 = lds_tr16(Lq + ct_lo_off(r0, trp)), l1 = lds_tr16(Lq + ct_lo_off(r0 + 4, trp));
                            const u32x4 b0 = {h0[0], h0[1], h1[0], h1[1]}, b1 = {m0[0], m0[1], m1[0], m1[1]},
                                        b2 = {l0[0], l0[1], l1[0], l1[1]};
                            CTX_MF6(dacc, wt.A0[k][ks], wt.A1[k][ks], wt.A2[k][ks], b0, b1, b2);
                        }
                    } else {
                        // K-step kk: dz rows 32 chf + 2 kk + h
                        const float* Sb = DZ + (p % RDZ) * CT_SET + (chf * 32 + h) * CT_F + (c & 3);
                        const int cpc = c >> 2;
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            const float b = Sb[kk * (2 * CT_F) + 4 * (cpc ^ (kk & 7))];
                            dacc = __builtin_amdgcn_mfma_f32_32x32x2f32(wt.af[k][kk], b, dacc, 0, 0, 0);
                        }
                    }
                }
                if (chf == 1) {
                    float* P = PART + ((q & 1) * 2 + cit) * 16 * 64 + lane;
#pragma unroll
                    for (int r = 0; r < 16; ++r) P[r * 64] = dacc[r];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();            // every LDS read of step q is done, partial sums are visible
                asm volatile("" ::: "memory");
                if (chf == 0) epilogue(q, n0);           // registers + LDS slots that stay valid during step q + 1
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                // the rings are reused by the next chunk
            asm volatile("" ::: "memory");
        }
        if (chf == 0 && a.partials) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s1 = half_wave_sum(st1[r]);
                const float s2 = half_wave_sum(st2[r]);
                const int row = cit * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (c == 0) {
                    float* pp = a.partials + ((size_t)blockIdx.x * CT_C + row) * 2;
                    pp[0] = s1;
                    pp[1] = s2;
                }
            }
        }
    }
}

template <int K, int S, bool X3>
int ct_launch(const trunet_convt_bwd_args* h, hipStream_t st) {
    constexpr size_t lds = CtLds<K, S, X3>::BYTES;
    auto kern = convt_bwd_kernel<K, S, X3>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3(CT_GRID), dim3(512), lds, st, *h);
    return trunet_launch_status();
}
template <int K, int S>
int ct_launch(const trunet_convt_bwd_args* h, hipStream_t st, bool x3) {
    return x3 ? ct_launch<K, S, true>(h, st) : ct_launch<K, S, false>(h, st);
}

}  // namespace

extern "C" int trunet_convt_bwd_nparts(void) { return CT_GRID; }

extern "C" int trunet_convt_bwd(const trunet_convt_bwd_args* h, void* stream) {
    if (!h || !h->dy || !h->z || !h->ca || !h->cb || !h->cc || !h->src || !h->s_scale || !h->s_shift || !h->s_mean ||
        !h->W || !h->dsrc || !h->partials || !h->w_partials)
        return TRUNET_EINVAL;
    if (h->NP <= 0 || (h->NP % TRUNET_TILE_FRAMES) != 0 || h->N <= 0 || h->N > h->NP || h->Lin <= 0 || h->w_numel <= 0)
        return TRUNET_EINVAL;
    if (h->Ci != CT_C || h->Co != CT_C) return TRUNET_ENOTSUP;
    if (h->pad != h->S / 2 || h->Lout != (h->Lin - 1) * h->S - 2 * h->pad + h->K) return TRUNET_EINVAL;
    // 32-bit byte offsets of the buffer stores: 36 channel rows of the gradient tensor below 2 GiB
    if ((size_t)h->Lin * h->NP * sizeof(float) * 36 >= ((size_t)1 << 31)) return TRUNET_ENOTSUP;
    hipStream_t st = (hipStream_t)stream;
    // the split path when it is on for the fused backward kernels, or for this kernel alone (diagnostic mode 8)
    const bool x3 = (trunet_gemm_x3_enable(-1) & (TRUNET_X3_BWD | 8)) != 0;
    if (h->K == 3 && h->S == 1) return ct_launch<3, 1>(h, st, x3);
    if (h->K == 3 && h->S == 2) return ct_launch<3, 2>(h, st, x3);
    if (h->K == 5 && h->S == 2) return ct_launch<5, 2>(h, st, x3);
    return TRUNET_ENOTSUP;
}
