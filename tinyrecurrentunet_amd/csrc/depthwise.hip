// Depthwise conv of DepthwiseSeparableConv1d (encoder.1-5; network.py:33-38 and its autograd), fp32 and bf16 octet layout.
//
// The window walk.  A thread owns a column (E elements wide) of every tensor and walks a chunk of its positions with a
// sliding window of rows in registers, so every tensor row is loaded exactly once:
//   forward   K rows of the activated input a = relu(sc zin + sh); the window moves by S rows per output row
//             z[lo] = b + sum_k w[k] a[lo S + k - K/2];
//   backward  groups of S input rows li = m S + e; the taps of a group touch the dz rows m - 1 .. m + 1
//             (dz = ca dy + cb z + cc, the BatchNorm backward of the conv's output), a 3-row window that moves by one row
//             per group; a compile-time rule picks the window row of every (e, tap).  Data gradient (masked by a > 0),
//             weight and bias gradient sums and the BatchNorm-backward sums of the result come out of the same pass;
//   backward, RZ  the same without reading z: z[m + 1] is recomputed from a window of activated input rows that the kernel
//             needs anyway, in the forward's order of operations, so it is the stored value bit for bit.
// The forward is written once over a layout trait (DwF32, DwBf16: what a thread owns, how a row is loaded and stored, which
// coefficient an element uses, how sums are accumulated and reduced); dw2_fwd and bdw_fwd are wrappers.  The fp32 backward is
// written once over RZ; dw2_bwd and dw2_bwd_rz are wrappers.  bdw_bwd_kernel is the same backward walk written out for the
// octet layout, sharing the dz-window rule (DwWin) and the helpers: built from one body with the fp32 backward, hipcc gave
// its <5, 2> instance 144-146 VGPRs instead of 123 (three waves per SIMD instead of four), whatever the formulation.
// The tap-gather pair at the end is the form for every other (K, S) and the TRUNET_DW_GATHER=1 A/B.
#include <stdlib.h>
#include "bf16_common.hpp"

namespace {

// every row is touched exactly once: non-temporal accesses keep them from evicting the neighbours' lines (same-box A/B:
// -0.4 ms per step fp32, -0.5 ms bf16; -DTRUNET_DW_TEMPORAL builds the default-policy form)
#ifndef TRUNET_DW_TEMPORAL
#define DW_LD(V, p) __builtin_nontemporal_load((const V*)(p))
#define DW_ST(V, p, v) __builtin_nontemporal_store((v), (V*)(p))
#else
#define DW_LD(V, p) (*(const V*)(p))
#define DW_ST(V, p, v) (*(V*)(p) = (v))
#endif

constexpr int DW2_FB = 32;                  // fp32: blocks over the frame quads (grid-stride)
constexpr int DW2_CH = 4;                   // fp32: position chunks
constexpr int DW2_PARTS = DW2_FB * DW2_CH;
__host__ __device__ inline int bdw_chunks(int rows) { return rows >= 32 ? 4 : (rows >= 16 ? 2 : 1); }   // bf16: position chunks

// put(i, sum over the block of v[i])
template <int NV, class F>
__device__ __forceinline__ void block_reduce(float (&v)[NV], float* smem /* [4][NV] */, F put) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float s = wave_sum(v[i]);
        if (lane == 0) smem[wave * NV + i] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NV; i += 256) put(i, (smem[i] + smem[NV + i]) + (smem[2 * NV + i] + smem[3 * NV + i]));
    __syncthreads();
}

// ---------------------------------------------------------------- the two layouts
// A layout object is one column: tensors are T[blockIdx.y][L][NP] with the column at offset n.  Sums of NV quantities per
// channel live in Acc[NC * NV], channel-major, and end up in a partials row [C][NV].

// fp32 [C][L][NP]: channel blockIdx.y, four frames.  Per-channel coefficients; padding frames masked per element; a row's
// four frames are summed in fp32, the running sums are fp64 (they feed cancelling BatchNorm expressions); grid-stride over
// the frame quads.
struct DwF32 {
    using T = float;
    using Acc = double;
    using Red = double;
    static constexpr int E = 4, NC = 1;
    static constexpr int red_len() { return 256; }
    int n, N;
    static __device__ __forceinline__ int ci(int) { return 0; }
    static __device__ __forceinline__ int chunks() { return DW2_CH; }
    __device__ __forceinline__ bool valid(int j) const { return n + j < N; }
    static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4 x = DW_LD(f32x4, p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x[j];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4], float (&stored)[4]) {
        const f32x4 x = {v[0], v[1], v[2], v[3]};
        DW_ST(f32x4, p, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) stored[j] = v[j];
    }
    // quantity i of the sums: r = f(j, r) over the elements (MASK: the valid ones)
    template <bool MASK, int NV, class F>
    __device__ __forceinline__ void fold(double (&s)[NV], int i, F f) const {
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!MASK || valid(j)) r = f(j, r);
        s[i] += (double)r;
    }
    // put(channel of the block, quantity, sum over the block)
    template <int NV, class F>
    static __device__ __forceinline__ void reduce(double (&s)[NV], double* red, F put) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const double r = block_sum_f64(s[i], red);
            if (threadIdx.x == 0) put(0, i, (float)r);
        }
    }
    template <class F>
    static __device__ __forceinline__ void columns(int NP, int N, F f) {
        for (int qd = blockIdx.x * 256 + threadIdx.x; qd < NP / 4; qd += DW2_FB * 256) f(DwF32{4 * qd, N});
    }
};

// bf16 octets [C/8][L][NP][8]: octet blockIdx.y, one frame.  Per-element coefficients; a padding frame is masked as a whole;
// statistics are taken from the ROUNDED stored value and folded straight into fp32 sums.
struct DwBf16 {
    using T = u32x4;
    using Acc = float;
    using Red = float;
    static constexpr int E = 8, NC = 8;
    static constexpr int red_len() { return 4 * 16; }
    int n, N;
    static __device__ __forceinline__ int ci(int j) { return j; }
    static __device__ __forceinline__ int chunks() { return gridDim.z; }
    __device__ __forceinline__ bool live() const { return n < N; }          // false: a padding frame
    static __device__ __forceinline__ void load(const u32x4* p, float (&v)[8]) { bf_unpack8(DW_LD(u32x4, p), v); }
    static __device__ __forceinline__ void store(u32x4* p, const float (&v)[8], float (&stored)[8]) {
        const u32x4 o = bf_pack8(v);
        DW_ST(u32x4, p, o);
        bf_unpack8(o, stored);
    }
    template <bool MASK, int NV, class F>
    __device__ __forceinline__ void fold(float (&s)[NV], int i, F f) const {
        static_assert(MASK, "the forward's statistics only: padding frames never count");
        if (live()) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j * (NV / 8) + i] = f(j, s[j * (NV / 8) + i]);
        }
    }
    template <int NV, class F>
    static __device__ __forceinline__ void reduce(float (&s)[NV], float* red, F put) {
        block_reduce<NV>(s, red, [&](int i, float v) { put(i / (NV / 8), i % (NV / 8), v); });
    }
    template <class F>
    static __device__ __forceinline__ void columns(int, int N, F f) {
        f(DwBf16{(int)(blockIdx.x * 256 + threadIdx.x), N});
    }
};

// per-channel coefficients of the block: NC of them from p[blockIdx.y * NC ..]
template <class Lay>
__device__ __forceinline__ void dw_coef(const float* __restrict__ p, float (&v)[Lay::NC]) {
#pragma unroll
    for (int j = 0; j < Lay::NC; ++j) v[j] = p[blockIdx.y * Lay::NC + j];
}
template <class Lay, int K>
__device__ __forceinline__ void dw_weights(const float* __restrict__ w, float (&wk)[Lay::NC][K]) {
#pragma unroll
    for (int j = 0; j < Lay::NC; ++j)
#pragma unroll
        for (int k = 0; k < K; ++k) wk[j][k] = w[(blockIdx.y * Lay::NC + j) * K + k];
}
// chunk blockIdx.z of `rows` rows
template <class Lay>
__device__ __forceinline__ void dw_chunk(int rows, int& r0, int& r1) {
    r0 = (int)(((long long)blockIdx.z * rows) / Lay::chunks());
    r1 = (int)(((long long)(blockIdx.z + 1) * rows) / Lay::chunks());
}
// act = relu(sc raw + sh) where ok, else 0
template <class Lay>
__device__ __forceinline__ void dw_activate(const float (&raw)[Lay::E], const float (&sc)[Lay::NC], const float (&sh)[Lay::NC],
                                            bool ok, float (&act)[Lay::E]) {
#pragma unroll
    for (int j = 0; j < Lay::E; ++j) act[j] = ok ? fmaxf(fmaf(raw[j], sc[Lay::ci(j)], sh[Lay::ci(j)]), 0.f) : 0.f;
}
// z = b + sum_k w[k] a[k]: the forward's order of operations
template <class Lay, int K>
__device__ __forceinline__ void dw_conv(const float (*a)[Lay::E], const float (&wk)[Lay::NC][K], const float (&bb)[Lay::NC],
                                        float (&z)[Lay::E]) {
#pragma unroll
    for (int j = 0; j < Lay::E; ++j) z[j] = bb[Lay::ci(j)];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < Lay::E; ++j) z[j] = fmaf(wk[Lay::ci(j)][k], a[k][j], z[j]);
}
template <int E>
__device__ __forceinline__ void dw_copy(float (&d)[E], const float (&s)[E]) {
#pragma unroll
    for (int j = 0; j < E; ++j) d[j] = s[j];
}

// ---------------------------------------------------------------- forward
// statistics (sum z, sum z^2 over the frames < N) -> partials[part][C][2], part = chunk * gridDim.x + blockIdx.x
template <int K, int S, class Lay, class T = typename Lay::T>
__device__ __forceinline__ void dw_fwd_body(const T* __restrict__ zin, const float* __restrict__ s_in,
                                            const float* __restrict__ t_in, const float* __restrict__ w,
                                            const float* __restrict__ b, T* __restrict__ zout, float* __restrict__ partials,
                                            int C, int Lin, int Lout, int NP, int N) {
    constexpr int E = Lay::E, NC = Lay::NC;
    __shared__ typename Lay::Red red[Lay::red_len()];
    float sc[NC], sh[NC], bb[NC], wk[NC][K];
    dw_coef<Lay>(s_in, sc); dw_coef<Lay>(t_in, sh); dw_coef<Lay>(b, bb);
    dw_weights<Lay, K>(w, wk);
    int lo0, lo1;
    dw_chunk<Lay>(Lout, lo0, lo1);
    typename Lay::Acc st[2 * NC] = {};
    Lay::columns(NP, N, [&](const Lay lay) {
        const T* src = zin + (size_t)blockIdx.y * Lin * NP + lay.n;
        T* dst = zout + (size_t)blockIdx.y * Lout * NP + lay.n;
        auto load_act = [&](int li, float (&act)[E]) {
            if (li >= 0 && li < Lin) {
                float v[E];
                Lay::load(src + (size_t)li * NP, v);
                dw_activate<Lay>(v, sc, sh, true, act);
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) act[j] = 0.f;
            }
        };
        float win[K][E];                // win[k] = activated input at li = lo*S + k - K/2
#pragma unroll
        for (int k = 0; k < K - S; ++k) load_act(lo0 * S + k - K / 2, win[k + S]);       // pre-shifted: the loop shifts first
        for (int lo = lo0; lo < lo1; ++lo) {
#pragma unroll
            for (int k = 0; k < K - S; ++k) dw_copy(win[k], win[k + S]);
#pragma unroll
            for (int k = K - S; k < K; ++k) load_act(lo * S + k - K / 2, win[k]);
            float acc[E], r[E];
            dw_conv<Lay, K>(win, wk, bb, acc);
            Lay::store(dst + (size_t)lo * NP, acc, r);
            lay.template fold<true>(st, 0, [&](int j, float s) { return s + r[j]; });
            lay.template fold<true>(st, 1, [&](int j, float s) { return fmaf(r[j], r[j], s); });
        }
    });
    const size_t row = (size_t)(blockIdx.z * gridDim.x + blockIdx.x) * C + blockIdx.y * NC;       // [part][C]
    Lay::reduce(st, red, [&](int j, int i, float v) { partials[(row + j) * 2 + i] = v; });
}

// ---------------------------------------------------------------- backward
// The dz window of the backward walk: groups of S input positions li = m*S + e; their taps touch the dz rows
// m + LOMIN .. m + LOMAX, kept in W window rows (row i = dz row m + LOMIN + i).
template <int K, int S>
struct DwWin {
    static_assert((K == 3 && S == 1) || (K == 5 && S == 2) || (K == 3 && S == 2), "window derived for these shapes");
    static constexpr int LOMIN = -1, LOMAX = 1, W = 3;
    // the window row that tap k of input row e reads, -1: the tap reads no dz row (compile-time after unrolling)
    static __device__ __forceinline__ constexpr int row(int e, int k) {
        const int num = e + K / 2 - k;                               // relative to m*S
        if (((num % S) + S) % S != 0) return -1;
        return ((num >= 0) ? num / S : -((-num) / S)) - LOMIN;
    }
};

// fp32 backward (the octet layout has its own text below: bdw_bwd_kernel).
// zs: the conv's raw output z (RZ == false) / unused; bias: the conv's bias (RZ == true) / unused.
// RZ: the window of activated input rows leads the group by K/2 + 1 rows:
//   aw[i] = a[m S + i], i < AW = S + K/2 + 1;   z[m + 1] = b + sum_k w[k] aw[S - K/2 + k]
// and a chunk warms up over two extra groups (dz rows m0 - 1 and m0).  Its loads are unconditional on clamped rows (a load
// inside a branch makes hipcc drain the memory queue in front of it).  The statistics' zin - mean comes from the activation
// where it is > 0 (elsewhere the masked gradient is 0): a = sc zin + sh.
// sums -> partials_in[part][C][2] (sum g, sum g (zin - mean)), w_partials[part][C][K], b_partials[part][C]
template <int K, int S, bool RZ>
__device__ __forceinline__ void dw2_bwd_body(const float* __restrict__ dy, const float* __restrict__ zs,
                                             const float* __restrict__ bias, const float* __restrict__ ca,
                                             const float* __restrict__ cb, const float* __restrict__ cc,
                                             const float* __restrict__ zin, const float* __restrict__ s_in,
                                             const float* __restrict__ t_in, const float* __restrict__ mean_in,
                                             const float* __restrict__ w, float* __restrict__ dy_in,
                                             float* __restrict__ partials_in, float* __restrict__ w_partials,
                                             float* __restrict__ b_partials, int C, int Lin, int Lout, int NP, int N) {
    using Win = DwWin<K, S>;
    constexpr int W = Win::W, E = DwF32::E;
    constexpr int AW = RZ ? S + K / 2 + 1 : 1, ZO = S - K / 2;
    __shared__ double red[DwF32::red_len()];
    const int c = blockIdx.y;
    const float a0 = ca[c], a1 = cb[c], a2 = cc[c];
    const float sc = s_in[c], sh = t_in[c], mu = mean_in[c], bb = RZ ? bias[c] : 0.f;
    float wk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wk[k] = w[c * K + k];
    // RZ, sc == 0 (BatchNorm weight exactly zero; uniform over the block): a does not carry zin, the row is read again.
    // (precision of a / sc - (sh / sc + mean): eps (|zin| + |sh / sc|); an offset beyond 2^16 times the scale: re-read as well)
    const bool sc0 = RZ && (fabsf(sc) < 1e-30f || fabsf(sh) > 65536.f * fabsf(sc));
    const float isc = sc0 ? 0.f : 1.f / sc, zoff = fmaf(sh, isc, mu);
    // per-thread sums; dwb: dw[0 .. K), db (db and st[0] cancel analytically in front of a BatchNorm)
    double st[2] = {}, dwb[K + 1] = {};
    int m0, m1;
    dw_chunk<DwF32>((Lin + S - 1) / S, m0, m1);
    DwF32::columns(NP, N, [&](const DwF32 lay) {
        const float* pdy = dy + (size_t)c * Lout * NP + lay.n;
        const float* pz = RZ ? nullptr : zs + (size_t)c * Lout * NP + lay.n;
        const float* pin = zin + (size_t)c * Lin * NP + lay.n;
        float* pout = dy_in + (size_t)c * Lin * NP + lay.n;
        auto activate = [&](const float (&raw)[E], bool ok, float (&act)[E]) {
#pragma unroll
            for (int j = 0; j < E; ++j) act[j] = ok ? fmaxf(fmaf(raw[j], sc, sh), 0.f) : 0.f;
        };
        // dz row from (dy, z): zero outside the tensor and in padding frames
        auto bn_bwd = [&](const float (&dv)[E], const float (&zv)[E], bool ok, float (&d)[E]) {
#pragma unroll
            for (int j = 0; j < E; ++j) d[j] = (ok && lay.valid(j)) ? fmaf(a0, dv[j], fmaf(a1, zv[j], a2)) : 0.f;
        };
        auto load_dz = [&](int lo, float (&d)[E]) {
            if (lo >= 0 && lo < Lout) {
                float dv[E], zv[E];
                DwF32::load(pdy + (size_t)lo * NP, dv);
                DwF32::load(pz + (size_t)lo * NP, zv);
                bn_bwd(dv, zv, true, d);
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) d[j] = 0.f;
            }
        };
        auto load_row = [&](int li, float (&act)[E]) {         // RZ: activated input row, unconditional clamped load
            float raw[E];
            DwF32::load(pin + (size_t)min(max(li, 0), Lin - 1) * NP, raw);
            activate(raw, li >= 0 && li < Lin, act);
        };
        float dzw[W][E];                // dzw[i] = dz row m + LOMIN + i
        float aw[AW][E];                // RZ: activated input rows m*S + i
        int ms = m0;
        if constexpr (RZ) {
#pragma unroll
            for (int i = 0; i < W; ++i)
#pragma unroll
                for (int j = 0; j < E; ++j) dzw[i][j] = 0.f;
            ms = m0 - 2;                // two warm-up groups: dz rows m0 - 1, m0
#pragma unroll
            for (int i = S; i < AW; ++i) load_row(ms * S + i - S, aw[i]);                // pre-shifted: the loop shifts first
        } else {
#pragma unroll
            for (int i = 1; i < W; ++i) load_dz(m0 + Win::LOMIN + i - 1, dzw[i]);        // pre-shifted
        }
        for (int m = ms; m < m1; ++m) {
            if constexpr (RZ) {
#pragma unroll
                for (int i = 0; i < AW - S; ++i) dw_copy(aw[i], aw[i + S]);
#pragma unroll
                for (int i = AW - S; i < AW; ++i) load_row(m * S + i, aw[i]);
            }
#pragma unroll
            for (int i = 0; i < W - 1; ++i) dw_copy(dzw[i], dzw[i + 1]);
            if constexpr (RZ) {
                const int lo = m + Win::LOMAX;
                float dv[E], zrec[E];
                DwF32::load(pdy + (size_t)min(max(lo, 0), Lout - 1) * NP, dv);
#pragma unroll
                for (int j = 0; j < E; ++j) zrec[j] = bb;             // dw2_fwd_kernel's order of operations
#pragma unroll
                for (int k = 0; k < K; ++k)
#pragma unroll
                    for (int j = 0; j < E; ++j) zrec[j] = fmaf(wk[k], aw[ZO + k][j], zrec[j]);
                bn_bwd(dv, zrec, lo >= 0 && lo < Lout, dzw[W - 1]);
                if (m < m0) continue;
            } else {
                load_dz(m + Win::LOMAX, dzw[W - 1]);
            }
            // the dz window is current
#pragma unroll
            for (int e = 0; e < S; ++e) {
                const int li = m * S + e;
                if (li >= Lin) continue;
                float act[E], zi[E], zc[E], g[E];                         // zc = zin - mean
                if constexpr (RZ) {
                    dw_copy(act, aw[e]);
#pragma unroll
                    for (int j = 0; j < E; ++j) zc[j] = fmaf(act[j], isc, -zoff);
                    if (sc0) {
                        DwF32::load(pin + (size_t)li * NP, zi);
#pragma unroll
                        for (int j = 0; j < E; ++j) zc[j] = zi[j] - mu;
                    }
                } else {
                    DwF32::load(pin + (size_t)li * NP, zi);
                    activate(zi, true, act);
                }
#pragma unroll
                for (int j = 0; j < E; ++j) g[j] = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int wi = Win::row(e, k);
                    if (wi < 0) continue;
#pragma unroll
                    for (int j = 0; j < E; ++j) g[j] = fmaf(wk[k], dzw[wi][j], g[j]);
                    lay.template fold<false>(dwb, k, [&](int j, float s) { return fmaf(dzw[wi][j], act[j], s); });
                    // the bias gradient: e == 0 here, every dz row counted once
                    if (k == K / 2) lay.template fold<false>(dwb, K, [&](int j, float s) { return s + dzw[wi][j]; });
                }
                float o[E], r[E];
#pragma unroll
                for (int j = 0; j < E; ++j) o[j] = (act[j] > 0.f) ? g[j] : 0.f;
                DwF32::store(pout + (size_t)li * NP, o, r);
                lay.template fold<false>(st, 0, [&](int j, float s) { return s + r[j]; });
                lay.template fold<false>(st, 1, [&](int j, float s) { return fmaf(r[j], RZ ? zc[j] : zi[j] - mu, s); });
            }
        }
    });
    const size_t row = (size_t)(blockIdx.z * gridDim.x + blockIdx.x) * C + c;                     // [part][C]
    DwF32::reduce(st, red, [&](int, int i, float v) { partials_in[row * 2 + i] = v; });
    DwF32::reduce(dwb, red, [&](int, int i, float v) {
        if (i < K) w_partials[row * K + i] = v;
        else b_partials[row] = v;
    });
}

// ---------------------------------------------------------------- the five window kernels
// fp32: grid (DW2_FB, C, DW2_CH); bf16: grid (NP / 256, C / 8, bdw_chunks(rows))
template <int K, int S>
__global__ __launch_bounds__(256) void dw2_fwd_kernel(const float* __restrict__ zin, const float* __restrict__ s_in,
                                                      const float* __restrict__ t_in, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ zout,
                                                      float* __restrict__ partials, int C, int Lin, int Lout, int NP, int N) {
    dw_fwd_body<K, S, DwF32>(zin, s_in, t_in, w, b, zout, partials, C, Lin, Lout, NP, N);
}

template <int K, int S>
__global__ __launch_bounds__(256) void dw2_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ ca,
    const float* __restrict__ cb, const float* __restrict__ cc, const float* __restrict__ zin,
    const float* __restrict__ s_in, const float* __restrict__ t_in, const float* __restrict__ mean_in,
    const float* __restrict__ w, float* __restrict__ dy_in, float* __restrict__ partials_in,
    float* __restrict__ w_partials, float* __restrict__ b_partials, int C, int Lin, int Lout, int NP, int N) {
    dw2_bwd_body<K, S, false>(dy, z, nullptr, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials,
                                    b_partials, C, Lin, Lout, NP, N);
}

// one of the four row passes of the stride-1 layers (dy, z, zin in; dy_in out) goes away for K FMAs per element
template <int K, int S>
__global__ __launch_bounds__(256) void dw2_bwd_rz_kernel(
    const float* __restrict__ dy, const float* __restrict__ bias, const float* __restrict__ ca,
    const float* __restrict__ cb, const float* __restrict__ cc, const float* __restrict__ zin,
    const float* __restrict__ s_in, const float* __restrict__ t_in, const float* __restrict__ mean_in,
    const float* __restrict__ w, float* __restrict__ dy_in, float* __restrict__ partials_in,
    float* __restrict__ w_partials, float* __restrict__ b_partials, int C, int Lin, int Lout, int NP, int N) {
    dw2_bwd_body<K, S, true>(dy, nullptr, bias, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials,
                                   b_partials, C, Lin, Lout, NP, N);
}

template <int K, int S>
__global__ __launch_bounds__(256) void bdw_fwd_kernel(const u32x4* __restrict__ zin, const float* __restrict__ s_in,
                                                      const float* __restrict__ t_in, const float* __restrict__ w,
                                                      const float* __restrict__ b, u32x4* __restrict__ zout,
                                                      float* __restrict__ partials, int C, int Lin, int Lout, int NP, int N) {
    dw_fwd_body<K, S, DwBf16>(zin, s_in, t_in, w, b, zout, partials, C, Lin, Lout, NP, N);
}

// the backward walk (DwWin) in the octet layout, written out: one octet, one frame; a padding frame loads no dz rows
template <int K, int S>
__global__ __launch_bounds__(256) void bdw_bwd_kernel(const u32x4* __restrict__ dy, const u32x4* __restrict__ z,
                                                      const float* __restrict__ ca, const float* __restrict__ cb,
                                                      const float* __restrict__ cc, const u32x4* __restrict__ zin,
                                                      const float* __restrict__ s_in, const float* __restrict__ t_in,
                                                      const float* __restrict__ mean_in, const float* __restrict__ w,
                                                      u32x4* __restrict__ dy_in, float* __restrict__ partials_in,
                                                      float* __restrict__ w_partials, float* __restrict__ b_partials, int C,
                                                      int Lin, int Lout, int NP, int N) {
    using Win = DwWin<K, S>;
    constexpr int W = Win::W;
    __shared__ float red[4 * 8 * (K + 1)];
    const int oct = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    int m0, m1;
    dw_chunk<DwBf16>((Lin + S - 1) / S, m0, m1);
    float a0[8], a1[8], a2[8], sc[8], sh[8], mu[8], wk[8][K];
    dw_coef<DwBf16>(ca, a0); dw_coef<DwBf16>(cb, a1); dw_coef<DwBf16>(cc, a2);
    dw_coef<DwBf16>(s_in, sc); dw_coef<DwBf16>(t_in, sh); dw_coef<DwBf16>(mean_in, mu);
    dw_weights<DwBf16, K>(w, wk);
    float st[16], dwb[8 * (K + 1)];       // dwb[j*(K+1) + k] = dw[j][k], [.. + K] = db[j]
#pragma unroll
    for (int j = 0; j < 16; ++j) st[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 8 * (K + 1); ++j) dwb[j] = 0.f;
    const u32x4* pdy = dy + (size_t)oct * Lout * NP + n;
    const u32x4* pz = z + (size_t)oct * Lout * NP + n;
    const u32x4* pin = zin + (size_t)oct * Lin * NP + n;
    u32x4* pout = dy_in + (size_t)oct * Lin * NP + n;
    const bool fin = n < N;
    auto load_dz = [&](int lo, float (&d)[8]) {
        if (lo >= 0 && lo < Lout && fin) {
            float dv[8], zv[8];
            bf_unpack8(DW_LD(u32x4, pdy + (size_t)lo * NP), dv);
            bf_unpack8(DW_LD(u32x4, pz + (size_t)lo * NP), zv);
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = fmaf(a0[j], dv[j], fmaf(a1[j], zv[j], a2[j]));
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) d[j] = 0.f;
        }
    };
    float dzw[W][8];                    // dzw[i] = dz row m + LOMIN + i
#pragma unroll
    for (int i = 1; i < W; ++i) load_dz(m0 + Win::LOMIN + i - 1, dzw[i]);            // pre-shifted
    for (int m = m0; m < m1; ++m) {
#pragma unroll
        for (int i = 0; i < W - 1; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) dzw[i][j] = dzw[i + 1][j];
        load_dz(m + Win::LOMAX, dzw[W - 1]);
#pragma unroll
        for (int e = 0; e < S; ++e) {
            const int li = m * S + e;
            if (li >= Lin) continue;
            float zi[8], act[8], g[8];
            bf_unpack8(DW_LD(u32x4, pin + (size_t)li * NP), zi);
#pragma unroll
            for (int j = 0; j < 8; ++j) { act[j] = fmaxf(fmaf(zi[j], sc[j], sh[j]), 0.f); g[j] = 0.f; }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int wi = Win::row(e, k);
                if (wi < 0) continue;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float dzv = dzw[wi][j];
                    g[j] = fmaf(wk[j][k], dzv, g[j]);
                    dwb[j * (K + 1) + k] = fmaf(dzv, act[j], dwb[j * (K + 1) + k]);
                    if (k == K / 2) dwb[j * (K + 1) + K] += dzv;     // e == 0 here: every dz row counted once
                }
            }
            float ov[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] = (act[j] > 0.f) ? g[j] : 0.f;
            const u32x4 o = bf_pack8(ov);
            DW_ST(u32x4, pout + (size_t)li * NP, o);
            float r[8];
            bf_unpack8(o, r);
#pragma unroll
            for (int j = 0; j < 8; ++j) { st[2 * j] += r[j]; st[2 * j + 1] = fmaf(r[j], zi[j] - mu[j], st[2 * j + 1]); }
        }
    }
    const int part = blockIdx.z * gridDim.x + blockIdx.x;
    block_reduce<16>(st, red, [&](int i, float v) { partials_in[((size_t)part * C + oct * 8) * 2 + i] = v; });
    block_reduce<8 * (K + 1)>(dwb, red, [&](int i, float v) {        // dw / db: [part][C][K] and [part][C]
        const int j = i / (K + 1), k = i - j * (K + 1);
        const int ch = oct * 8 + j;
        if (k < K) w_partials[((size_t)part * C + ch) * K + k] = v;
        else b_partials[(size_t)part * C + ch] = v;
    });
}

// ---------------------------------------------------------------- tap-gather form, any (K, S): one statistics row per block
template <int K>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ zin, const float* __restrict__ s_in,
                                                         const float* __restrict__ t_in, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ zout,
                                                         float* __restrict__ partials, int C, int S, int Lin, int Lout,
                                                         int NP, int N) {
    __shared__ double red[256];
    const int c = blockIdx.y;
    const int f4 = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float sc = s_in[c], sh = t_in[c], bb = b[c];
    float wk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wk[k] = w[c * K + k];
    const int ntn = NP / 128;
    const int items = Lout * ntn;
    float s1 = 0.f, s2 = 0.f;
    for (int it = blockIdx.x * 8 + ly; it < items; it += gridDim.x * 8) {
        const int nt = it / Lout, lo = it - nt * Lout;
        const int n = nt * 128 + 4 * f4;
        f32x4 acc = {bb, bb, bb, bb};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int li = lo * S + k - K / 2;
            if (li >= 0 && li < Lin) {
                f32x4 v = *(const f32x4*)(zin + ((size_t)c * Lin + li) * NP + n);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wk[k], fmaxf(fmaf(v[e], sc, sh), 0.f), acc[e]);
            }
        }
        *(f32x4*)(zout + ((size_t)c * Lout + lo) * NP + n) = acc;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (n + e < N) { s1 += acc[e]; s2 = fmaf(acc[e], acc[e], s2); }
    }
    double r1 = block_sum_f64((double)s1, red);
    double r2 = block_sum_f64((double)s2, red);
    if (threadIdx.x == 0) {
        partials[((size_t)blockIdx.x * C + c) * 2 + 0] = (float)r1;
        partials[((size_t)blockIdx.x * C + c) * 2 + 1] = (float)r2;
    }
}

template <int K>
__global__ __launch_bounds__(256) void dwconv_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ ca,
    const float* __restrict__ cb, const float* __restrict__ cc, const float* __restrict__ zin,
    const float* __restrict__ s_in, const float* __restrict__ t_in, const float* __restrict__ mean_in,
    const float* __restrict__ w, float* __restrict__ dy_in, float* __restrict__ partials_in,
    float* __restrict__ w_partials, float* __restrict__ b_partials, int C, int S, int Lin, int Lout, int NP, int N) {
    __shared__ double red[256];
    const int c = blockIdx.y;
    const int f4 = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float a0 = ca[c], a1 = cb[c], a2 = cc[c];
    const float sc = s_in[c], sh = t_in[c], mu = mean_in[c];
    float wk[K], dwk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { wk[k] = w[c * K + k]; dwk[k] = 0.f; }
    float db = 0.f, s1 = 0.f, s2 = 0.f;
    const int ntn = NP / 128;
    const int items = Lin * ntn;
    for (int it = blockIdx.x * 8 + ly; it < items; it += gridDim.x * 8) {
        const int nt = it / Lin, li = it - nt * Lin;
        const int n = nt * 128 + 4 * f4;
        const f32x4 zi = *(const f32x4*)(zin + ((size_t)c * Lin + li) * NP + n);
        f32x4 act, g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) act[e] = fmaxf(fmaf(zi[e], sc, sh), 0.f);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int num = li + K / 2 - k;
            const int lo = num / S;
            if (num >= 0 && lo * S == num && lo < Lout) {
                const size_t off = ((size_t)c * Lout + lo) * NP + n;
                const f32x4 dv = *(const f32x4*)(dy + off);
                const f32x4 zv = *(const f32x4*)(z + off);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float dz = (n + e < N) ? fmaf(a0, dv[e], fmaf(a1, zv[e], a2)) : 0.f;
                    g[e] = fmaf(wk[k], dz, g[e]);
                    dwk[k] = fmaf(dz, act[e], dwk[k]);
                    if (k == K / 2) db += dz;
                }
            }
        }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (act[e] > 0.f) ? g[e] : 0.f;
            s1 += o[e];
            s2 = fmaf(o[e], zi[e] - mu, s2);
        }
        *(f32x4*)(dy_in + ((size_t)c * Lin + li) * NP + n) = o;
    }
    double r;
    r = block_sum_f64((double)s1, red);
    if (threadIdx.x == 0) partials_in[((size_t)blockIdx.x * C + c) * 2 + 0] = (float)r;
    r = block_sum_f64((double)s2, red);
    if (threadIdx.x == 0) partials_in[((size_t)blockIdx.x * C + c) * 2 + 1] = (float)r;
    r = block_sum_f64((double)db, red);
    if (threadIdx.x == 0) b_partials[(size_t)blockIdx.x * C + c] = (float)r;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r = block_sum_f64((double)dwk[k], red);
        if (threadIdx.x == 0) w_partials[((size_t)blockIdx.x * C + c) * K + k] = (float)r;
    }
}

// ---------------------------------------------------------------- launchers
template <int K_, int S_>
struct DwShape { static constexpr int K = K_, S = S_; };

// f(DwShape<K, S>) for the (K, S) the window kernels are built for; false for any other
template <class F>
bool dw_dispatch(int K, int S, F f) {
    if (K == 3 && S == 1) f(DwShape<3, 1>{});
    else if (K == 5 && S == 2) f(DwShape<5, 2>{});
    else if (K == 3 && S == 2) f(DwShape<3, 2>{});
    else return false;
    return true;
}
template <class... P>
bool dw_all_set(P... p) { return (... && (p != nullptr)); }
// 'same' padding K/2 (S > 0 is the caller's business, as it has been)
bool dw_lout_ok(int K, int S, int Lin, int Lout) { return Lout == (Lin + 2 * (K / 2) - K) / S + 1; }

// TRUNET_DW_GATHER=1: the tap-gather kernels for every shape (A/B measurements)
bool dw_gather_forced() {
    static const bool v = [] { const char* e = getenv("TRUNET_DW_GATHER"); return e && e[0] == '1'; }();
    return v;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_dwconv_nparts(int Lout) { (void)Lout; return DW2_PARTS; }
extern "C" int trunet_dwconv_bwd_nparts(int Lin) { (void)Lin; return DW2_PARTS; }
extern "C" int trunet_bf16_dw_nparts(int NP, int rows) { return (NP / 256) * bdw_chunks(rows); }

extern "C" int trunet_dwconv_fwd(const float* zin, const float* s_in, const float* t_in, const float* w, const float* b,
                                 float* zout, float* partials, int C, int K, int S, int Lin, int Lout, int NP, int N,
                                 void* stream) {
    if (!dw_all_set(zin, s_in, t_in, w, b, zout, partials) || (NP % 128)) return TRUNET_EINVAL;
    if (!dw_gather_forced() && dw_lout_ok(K, S, Lin, Lout) && dw_dispatch(K, S, [&](auto ks) {
            hipLaunchKernelGGL((dw2_fwd_kernel<decltype(ks)::K, decltype(ks)::S>), dim3(DW2_FB, C, DW2_CH), dim3(256), 0, ST, zin,
                               s_in, t_in, w, b, zout, partials, C, Lin, Lout, NP, N);
        }))
        return trunet_launch_status();
    dim3 grid(DW2_PARTS, C);            // other shapes: the tap-gather form, one statistics row per block as well
    if (K == 3) hipLaunchKernelGGL(dwconv_fwd_kernel<3>, grid, dim3(256), 0, ST, zin, s_in, t_in, w, b, zout, partials, C, S, Lin, Lout, NP, N);
    else if (K == 5) hipLaunchKernelGGL(dwconv_fwd_kernel<5>, grid, dim3(256), 0, ST, zin, s_in, t_in, w, b, zout, partials, C, S, Lin, Lout, NP, N);
    else return TRUNET_ENOTSUP;
    return trunet_launch_status();
}

extern "C" int trunet_dwconv_bwd(const float* dy, const float* z, const float* ca, const float* cb, const float* cc,
                                 const float* zin, const float* s_in, const float* t_in, const float* mean_in,
                                 const float* w, float* dy_in, float* partials_in, float* w_partials, float* b_partials,
                                 int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream) {
    if (!dw_all_set(dy, z, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials) || (NP % 128))
        return TRUNET_EINVAL;
    if (!dw_gather_forced() && dw_lout_ok(K, S, Lin, Lout) && dw_dispatch(K, S, [&](auto ks) {
            hipLaunchKernelGGL((dw2_bwd_kernel<decltype(ks)::K, decltype(ks)::S>), dim3(DW2_FB, C, DW2_CH), dim3(256), 0, ST, dy,
                               z, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials, C, Lin,
                               Lout, NP, N);
        }))
        return trunet_launch_status();
    dim3 grid(DW2_PARTS, C);
    if (K == 3) hipLaunchKernelGGL(dwconv_bwd_kernel<3>, grid, dim3(256), 0, ST, dy, z, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials, C, S, Lin, Lout, NP, N);
    else if (K == 5) hipLaunchKernelGGL(dwconv_bwd_kernel<5>, grid, dim3(256), 0, ST, dy, z, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials, C, S, Lin, Lout, NP, N);
    else return TRUNET_ENOTSUP;
    return trunet_launch_status();
}

// trunet_dwconv_bwd without the z operand: z is recomputed from (zin, w, bias) as trunet_dwconv_fwd computed it
// (TRUNET_ENOTSUP for shapes the sliding-window kernels do not cover: call trunet_dwconv_bwd with z then)
extern "C" int trunet_dwconv_bwd_rz(const float* dy, const float* bias, const float* ca, const float* cb, const float* cc,
                                    const float* zin, const float* s_in, const float* t_in, const float* mean_in,
                                    const float* w, float* dy_in, float* partials_in, float* w_partials, float* b_partials,
                                    int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream) {
    if (!dw_all_set(dy, bias, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials) || (NP % 128))
        return TRUNET_EINVAL;
    static const bool off = [] { const char* e = getenv("TRUNET_DW_RZ"); return e && e[0] == '0'; }();
    if (off || dw_gather_forced() || !dw_lout_ok(K, S, Lin, Lout)) return TRUNET_ENOTSUP;
    // few output positions: the two warm-up groups per chunk and the four-row window cost more than the z row they save
    // (encoder.5, k3 s2, 32 -> 16 positions: 331 us against 308 us for the z-reading kernel)
    if (Lout < 32 && !(getenv("TRUNET_DW_RZ") && getenv("TRUNET_DW_RZ")[0] == '2')) return TRUNET_ENOTSUP;
    if (!dw_dispatch(K, S, [&](auto ks) {
            hipLaunchKernelGGL((dw2_bwd_rz_kernel<decltype(ks)::K, decltype(ks)::S>), dim3(DW2_FB, C, DW2_CH), dim3(256), 0, ST, dy,
                               bias, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials, C, Lin, Lout,
                               NP, N);
        }))
        return TRUNET_ENOTSUP;
    return trunet_launch_status();
}

// bf16 octet layout (TRUNET_ENOTSUP outside the three window shapes: there is no gather form)
static bool bdw_args_ok(int C, int K, int S, int Lin, int Lout, int NP, int N) {
    return C > 0 && !(C % 8) && NP > 0 && !(NP % 256) && N > 0 && N <= NP && Lin > 0 && dw_lout_ok(K, S, Lin, Lout);
}

extern "C" int trunet_bf16_dwconv_fwd(const void* zin, const float* s_in, const float* t_in, const float* w, const float* b,
                                      void* zout, float* partials, int C, int K, int S, int Lin, int Lout, int NP, int N,
                                      void* stream) {
    if (!dw_all_set(zin, s_in, t_in, w, b, zout, partials) || !bdw_args_ok(C, K, S, Lin, Lout, NP, N)) return TRUNET_EINVAL;
    if (!dw_dispatch(K, S, [&](auto ks) {
            hipLaunchKernelGGL((bdw_fwd_kernel<decltype(ks)::K, decltype(ks)::S>), dim3(NP / 256, C / 8, bdw_chunks(Lout)),
                               dim3(256), 0, ST, (const u32x4*)zin, s_in, t_in, w, b, (u32x4*)zout, partials, C, Lin, Lout, NP, N);
        }))
        return TRUNET_ENOTSUP;
    return trunet_launch_status();
}

extern "C" int trunet_bf16_dwconv_bwd(const void* dy, const void* z, const float* ca, const float* cb, const float* cc,
                                      const void* zin, const float* s_in, const float* t_in, const float* mean_in,
                                      const float* w, void* dy_in, float* partials_in, float* w_partials, float* b_partials,
                                      int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream) {
    if (!dw_all_set(dy, z, ca, cb, cc, zin, s_in, t_in, mean_in, w, dy_in, partials_in, w_partials, b_partials) ||
        !bdw_args_ok(C, K, S, Lin, Lout, NP, N))
        return TRUNET_EINVAL;
    if (!dw_dispatch(K, S, [&](auto ks) {
            hipLaunchKernelGGL((bdw_bwd_kernel<decltype(ks)::K, decltype(ks)::S>), dim3(NP / 256, C / 8, bdw_chunks(Lin)),
                               dim3(256), 0, ST, (const u32x4*)dy, (const u32x4*)z, ca, cb, cc, (const u32x4*)zin, s_in, t_in,
                               mean_in, w, (u32x4*)dy_in, partials_in, w_partials, b_partials, C, Lin, Lout, NP, N);
        }))
        return TRUNET_ENOTSUP;
    return trunet_launch_status();
}
