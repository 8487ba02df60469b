// The frame layout and the vector-ALU helpers of the single-launch eval forward, shared by stream_fwd.hip (fp32 and split-bf16
// MFMA; its header explains the layout) and stream_fwd_i8.hip (int8 MFMA).  A workgroup of SF_T threads takes one frame at a
// time through the network in its 160 KiB of LDS; the skip tensors go to a per-workgroup region of the scratch buffer.
#pragma once
#include "common.hpp"

namespace {

constexpr int SF_T = 256;
constexpr int SF_R0 = 0, SF_R1A = 18432, SF_R1B = 18432 + 9216, SF_R2 = 36864, SF_ARENA = 40960;   // floats (160 KiB)
// small fixed buffers behind the three activation regions: features of the frame, first-conv weights (resident for the
// whole kernel), depthwise / last-layer weights of the current block, GRU state
constexpr int SF_XB = SF_R2, SF_W0 = SF_R2 + 1088, SF_DWB = SF_R2 + 2432, SF_GRU = SF_R2 + 3200;
constexpr int SF_SKIP = 8192 + 16384 + 8192 + 8192 + 4096;       // enc0..enc4 per workgroup (floats)

__host__ __device__ constexpr int sf_ls(int L) { return (L + 8 + 15) / 16 * 16; }

constexpr int LSA = sf_ls(128);          // one row stride (144 floats) for every activation buffer: immediate LDS offsets
constexpr int LSG = sf_ls(16);           // ... except the GRU projection [384][32]

#ifndef GRU_LIBM
__device__ __forceinline__ float sf_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float sf_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }
#else
__device__ __forceinline__ float sf_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float sf_tanh(float x) { return tanhf(x); }
#endif

__device__ __forceinline__ float sf_dpp_xor1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}

// The per-lane addresses of a layer's epilogue depend only on the thread index, so the compiler would compute them for
// all layers once, before the frame loop, and keep (spill) hundreds of them: every layer re-derives them from an opaque
// copy of the thread index instead.
__device__ __forceinline__ int sf_tid() {
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// zero the guard columns [-4, 0) and [L, L + 4) of a [rows][ls] buffer
__device__ __forceinline__ void sf_guards(float* lds, int buf, int rows, int ls, int L) {
    for (int i = sf_tid(); i < rows * 8; i += SF_T) {
        const int r = i >> 3, g = i & 7;
        lds[buf + r * ls + (g < 4 ? g : L + g)] = 0.f;
    }
}

// depthwise conv (k = K, stride S, padding K/2) + folded BatchNorm + ReLU; weights staged in LDS at `wl` ([C][K] then [C]).
// A lane produces 4 consecutive outputs of one channel row from the 16-byte quads that cover its input window
// (conflict-free: consecutive lanes read consecutive quads of a row).  Lout is a multiple of 4.
template <int K, int S>
__device__ __forceinline__ void sf_dw(float* lds, int src, int lsi, int dst, int lsd, int wl, int C, int Lout) {
    constexpr int NQ = (3 * S + K - 1 + K / 2 + 3) / 4 + 1;      // quads from 4 (j S - 1) on: covers [4 j S - K/2, 4 j S + 3 S + K/2]
    const int Q = Lout >> 2;
    for (int o = sf_tid(); o < C * Q; o += SF_T) {
        const int ch = o / Q, j = o - ch * Q;
        float w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = lds[wl + ch * K + k];
        const float b = lds[wl + C * K + ch];
        float in[4 * NQ];
        const float* ip = lds + src + ch * lsi + 4 + 4 * j * S - 4;        // 16-byte aligned
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const f32x4 t = *(const f32x4*)(ip + 4 * q);
            in[4 * q] = t[0]; in[4 * q + 1] = t[1]; in[4 * q + 2] = t[2]; in[4 * q + 3] = t[3];
        }
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = b;
#pragma unroll
            for (int k = 0; k < K; ++k) v = fmaf(w[k], in[4 + e * S + k - K / 2], v);     // column 4 j S + e S + k - K/2
            r[e] = fmaxf(v, 0.f);
        }
        *(f32x4*)(lds + dst + ch * lsd + 4 + 4 * j) = r;
    }
}

// [C][L] dense (global scratch) <-> LDS buffer rows, 16 bytes per access; L = 4 << lq (rows start 16-byte aligned)
__device__ __forceinline__ void sf_save(const float* lds, int buf, int ls, float* g, int C, int lq) {
    for (int i = sf_tid(); i < (C << lq); i += SF_T) {
        const int ch = i >> lq, q = i - (ch << lq);
        ((f32x4*)g)[i] = *(const f32x4*)(lds + buf + ch * ls + 4 + 4 * q);
    }
}
// the same in two halves: up to 16 quads per thread are requested (registers) before a compute phase and written to LDS
// after it, so the L2 / Infinity-Cache latency of the skip tensor hides behind that phase
__device__ __forceinline__ void sf_restore_request(f32x4 (&rr)[16], const float* g, int C, int lq) {
    const int t = sf_tid();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = t + SF_T * j;
        if (i < (C << lq)) rr[j] = ((const f32x4*)g)[i];
    }
}
__device__ __forceinline__ void sf_restore_commit(const f32x4 (&rr)[16], float* lds, int buf, int ls, int C, int lq) {
    const int t = sf_tid();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = t + SF_T * j;
        if (i < (C << lq)) {
            const int ch = i >> lq, q = i - (ch << lq);
            *(f32x4*)(lds + buf + ch * ls + 4 + 4 * q) = rr[j];
        }
    }
    sf_guards(lds, buf, C, ls, 4 << lq);
}
__device__ __forceinline__ void sf_restore(float* lds, int buf, int ls, const float* g, int C, int lq) {
    for (int i = sf_tid(); i < (C << lq); i += SF_T) {
        const int ch = i >> lq, q = i - (ch << lq);
        *(f32x4*)(lds + buf + ch * ls + 4 + 4 * q) = ((const f32x4*)g)[i];
    }
    sf_guards(lds, buf, C, ls, 4 << lq);
}
}  // namespace
