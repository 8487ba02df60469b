// Memory-bound stages of the TRU-Net body in the frames-last layout: layout changes, the first
// (C_in -> 64) strided conv, BatchNorm statistics -> affine, AdamW (the depthwise convs: depthwise.hip).
// All are HBM-bound: coalesced 16-byte accesses along the frame axis, one pass per tensor.
#include "common.hpp"

namespace {

// ---------------------------------------------------------------- layout changes
// X[N][R] (R = C*L contiguous per frame)  <->  Y[R][NP]
__global__ void to_frames_last_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int R, int NP) {
    __shared__ float t[32][33];
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        int n = n0 + i, r = r0 + tx;
        t[i][tx] = (n < N && r < R) ? x[(size_t)n * R + r] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int r = r0 + i, n = n0 + tx;
        if (r < R && n < NP) y[(size_t)r * NP + n] = t[tx][i];
    }
}

__global__ void from_frames_last_kernel(const float* __restrict__ y, float* __restrict__ x, int N, int R, int NP) {
    __shared__ float t[32][33];
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        int r = r0 + i, n = n0 + tx;
        t[i][tx] = (r < R && n < NP) ? y[(size_t)r * NP + n] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int n = n0 + i, r = r0 + tx;
        if (n < N && r < R) x[(size_t)n * R + r] = t[tx][i];
    }
}

// Y[R][NP] -> X[N][R] with the consumer-side BatchNorm+ReLU applied on the way out (block outputs of the
// reference API are post-activation): x = max(scale[c]*y + shift[c], lo), c = r / L
__global__ void from_frames_last_affine_kernel(const float* __restrict__ y, float* __restrict__ x, int N, int R, int NP,
                                               int L, const float* __restrict__ scale, const float* __restrict__ shift,
                                               float lo) {
    __shared__ float t[32][33];
    const int n0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        int r = r0 + i, n = n0 + tx;
        float v = 0.f;
        if (r < R && n < NP) {
            const int c = r / L;
            v = fmaxf(fmaf(y[(size_t)r * NP + n], scale[c], shift[c]), lo);
        }
        t[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        int n = n0 + i, r = r0 + tx;
        if (n < N && r < R) x[(size_t)n * R + r] = t[tx][i];
    }
}

// ---------------------------------------------------------------- first conv (+ReLU)
// y[co][lo][n] = relu(b[co] + sum_{ci,k} w[co][ci][k] * x[ci][lo*S + k - S/2][n])
template <int CIN, int K>
__global__ __launch_bounds__(256) void conv_first_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ b, float* __restrict__ y, int Cout,
                                                         int S, int Lin, int Lout, int NP) {
    const int f4 = threadIdx.x;                 // 32 lanes x float4 = 128 frames
    const int lo = blockIdx.y * 8 + threadIdx.y;
    const size_t n = (size_t)blockIdx.x * 128 + 4 * f4;
    if (lo >= Lout) return;
    f32x4 xv[CIN][K];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int li = lo * S + k - S / 2;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            xv[ci][k] = (li >= 0 && li < Lin) ? *(const f32x4*)(x + ((size_t)ci * Lin + li) * NP + n) : z;
        }
    for (int co = 0; co < Cout; ++co) {
        const float bb = b[co];
        f32x4 acc = {bb, bb, bb, bb};
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float wv = w[(co * CIN + ci) * K + k];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv, xv[ci][k][e], acc[e]);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
#ifdef TRUNET_THIN_NT
        __builtin_nontemporal_store(acc, (f32x4*)(y + ((size_t)co * Lout + lo) * NP + n));
#else
        *(f32x4*)(y + ((size_t)co * Lout + lo) * NP + n) = acc;
#endif
    }
}

// ---------------------------------------------------------------- activation backward at a block boundary
constexpr int DW_PARTS = 16;
// A stand-alone block class (network.py:9-120) receives the cotangent of its POST-activation output, the fused
// schedule works on gradients of the BatchNorm output: dy *= [sc[c] z + sh[c] > 0] in place (sc == NULL: [z > 0],
// StandardConv1d's plain ReLU) and, with mean != NULL, the BatchNorm-backward sums of the result
// (sum dy, sum dy (z - mean[c])) -> partials[DW_PARTS][C][2].
__global__ __launch_bounds__(256) void relu_bwd_stats_kernel(float* __restrict__ dy, const float* __restrict__ z,
                                                             const float* __restrict__ sc, const float* __restrict__ sh,
                                                             const float* __restrict__ mean, float* __restrict__ partials,
                                                             int C, int L, int NP, int N) {
    __shared__ double red[256];
    const int c = blockIdx.y;
    const int f4 = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const float a0 = sc ? sc[c] : 1.f, a1 = sc ? sh[c] : 0.f, mu = mean ? mean[c] : 0.f;
    const int ntn = NP / 128;
    const int items = L * ntn;
    float s1 = 0.f, s2 = 0.f;
    for (int it = blockIdx.x * 8 + ly; it < items; it += gridDim.x * 8) {
        const int nt = it / L, l = it - nt * L;
        const int n = nt * 128 + 4 * f4;
        const size_t off = ((size_t)c * L + l) * NP + n;
        f32x4 d = *(const f32x4*)(dy + off);
        const f32x4 zv = *(const f32x4*)(z + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            d[e] = (n + e < N && fmaf(zv[e], a0, a1) > 0.f) ? d[e] : 0.f;
            s1 += d[e];
            s2 = fmaf(d[e], (n + e < N) ? zv[e] - mu : 0.f, s2);
        }
        *(f32x4*)(dy + off) = d;
    }
    if (partials) {
        double r = block_sum_f64((double)s1, red);
        if (threadIdx.x == 0) partials[((size_t)blockIdx.x * C + c) * 2 + 0] = (float)r;
        r = block_sum_f64((double)s2, red);
        if (threadIdx.x == 0) partials[((size_t)blockIdx.x * C + c) * 2 + 1] = (float)r;
    }
}

// ---------------------------------------------------------------- one GRU time step (streaming TGRU)
// gi = W_ih x + b_ih, gh = W_hh h + b_hh as [3H][R] rows (R = L*NP contiguous), torch gate order r, z, n:
//   r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) n + z h
__global__ __launch_bounds__(256) void gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                       const float* h, float* hn, int H,   // h may alias hn
                                                      
                                                       size_t R4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // float4 index inside one row block [H][R]
    if (i >= (size_t)H * R4) return;
    const size_t HR = (size_t)H * R4;
    const f32x4* gi4 = (const f32x4*)gi;
    const f32x4* gh4 = (const f32x4*)gh;
    const f32x4 ir = gi4[i], iz = gi4[HR + i], in_ = gi4[2 * HR + i];
    const f32x4 hr = gh4[i], hz = gh4[HR + i], hn_ = gh4[2 * HR + i];
    const f32x4 hp = ((const f32x4*)h)[i];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float r = 1.f / (1.f + expf(-(ir[e] + hr[e])));
        const float z = 1.f / (1.f + expf(-(iz[e] + hz[e])));
        const float n = tanhf(in_[e] + r * hn_[e]);
        o[e] = (1.f - z) * n + z * hp[e];
    }
    ((f32x4*)hn)[i] = o;
}

// ---------------------------------------------------------------- TGRU: sequence-major layout and the time loop's cells
// frames-last x[c][l][b*T + t]  <->  sequence-major y[c][t][s], s = b*Lf + l (every (utterance, frequency position) is
// one sequence of the time-recurrent block, network.py:150).  32 x 32 (t, s... ) tiles through LDS; block = (32, 8).
// to: y = max(sc[c] x + sh[c], lo) (BatchNorm+ReLU of the source, or identity when sc == NULL).  The kernel writes the
// sequences s < S = B*Lf only; y = 0 for s in [S, SP) comes from trunet_to_seq_major, which zero-fills all of y in front of
// the launch (the padded sequences feed whole-tile GEMMs and the recurrence, so they must be finite).
__global__ void to_seq_major_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ sc,
                                    const float* __restrict__ sh, int Lf, int T, int B, int NP, int SP, float lo) {
    __shared__ float tl[32][33];
    const int c = blockIdx.z / Lf, l = blockIdx.z % Lf;
    const int t0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const float a0 = sc ? sc[c] : 1.f, a1 = sc ? sh[c] : 0.f;
    for (int i = ty; i < 32; i += 8) {          // read: t contiguous
        const int b = b0 + i, t = t0 + tx;
        float v = 0.f;
        if (b < B && t < T) v = fmaxf(fmaf(x[((size_t)c * Lf + l) * NP + (size_t)b * T + t], a0, a1), lo);
        tl[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {          // write: b varies fastest -> stride Lf in s
        const int t = t0 + i, b = b0 + tx;
        if (t < T && b < B) y[((size_t)c * T + t) * SP + (size_t)b * Lf + l] = tl[tx][i];
    }
}

// from: x[c][l][b*T + t] = y[c][t][s] (raw), or with zsrc != NULL the backward of `to` with its BatchNorm+ReLU:
// x = y * [sc z + sh > 0] plus per-block partial sums (sum x, sum x (z - mean)) -> partials[(blk)][C][2].
__global__ void from_seq_major_kernel(const float* __restrict__ y, float* __restrict__ x, const float* __restrict__ zsrc,
                                      const float* __restrict__ sc, const float* __restrict__ sh,
                                      const float* __restrict__ mean, float* __restrict__ partials, int C, int Lf, int T,
                                      int B, int NP, int SP) {
    __shared__ float tl[32][33];
    __shared__ float red[2][8];
    const int c = blockIdx.z / Lf, l = blockIdx.z % Lf;
    const int t0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, b = b0 + tx;
        tl[tx][i] = (t < T && b < B) ? y[((size_t)c * T + t) * SP + (size_t)b * Lf + l] : 0.f;
    }
    __syncthreads();
    float s1 = 0.f, s2 = 0.f;
    const float a0 = zsrc ? sc[c] : 0.f, a1 = zsrc ? sh[c] : 0.f, mu = zsrc ? mean[c] : 0.f;
    for (int i = ty; i < 32; i += 8) {
        const int b = b0 + i, t = t0 + tx;
        if (b < B && t < T) {
            const size_t o = ((size_t)c * Lf + l) * NP + (size_t)b * T + t;
            float v = tl[i][tx];
            if (zsrc) {
                const float z = zsrc[o];
                v = (fmaf(a0, z, a1) > 0.f) ? v : 0.f;
                s1 += v;
                s2 = fmaf(v, z - mu, s2);
            }
            x[o] = v;
        }
    }
    if (zsrc) {
        // reduce over the 32 lanes of a row (threadIdx.x), then over the 8 rows
        for (int m = 16; m > 0; m >>= 1) { s1 += __shfl_xor(s1, m, 32); s2 += __shfl_xor(s2, m, 32); }
        if (tx == 0) { red[0][ty] = s1; red[1][ty] = s2; }
        __syncthreads();
        if (tx == 0 && ty == 0) {
            float r1 = 0.f, r2 = 0.f;
            for (int i = 0; i < 8; ++i) { r1 += red[0][i]; r2 += red[1][i]; }
            // one partial row per (t block, b block, l): blocks of the same channel never collide
            const size_t blk = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * Lf + l;
            partials[(blk * C + c) * 2 + 0] = r1;
            partials[(blk * C + c) * 2 + 1] = r2;
        }
    }
}

// time step t of nn.GRU forward on sequence-major tensors: gi_all [3H][T][SP] (= W_ih x + b_ih), gh [3H][SP]
// (= W_hh h_{t-1} + b_hh), hs [H][T+1][SP] with hs[:, 0] = h_{-1} = 0 and h_t at position t+1;
// gates [4][H][T][SP] = r, z, n, gh_n (training; may be NULL).
__global__ __launch_bounds__(256) void tgru_cell_fwd_kernel(const float* __restrict__ gi_all, const float* __restrict__ gh,
                                                            float* hs, float* __restrict__ gates, int H, int T, int t,
                                                            int SP) {
    const int s4 = SP / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * s4) return;
    const int j = (int)(i / s4), q = (int)(i % s4);
    const f32x4* gi4 = (const f32x4*)gi_all;
    const f32x4* gh4 = (const f32x4*)gh;
    const size_t grow = (size_t)T * s4;                       // float4 stride between rows of gi_all
    const f32x4 ir = gi4[(size_t)j * grow + (size_t)t * s4 + q];
    const f32x4 iz = gi4[(size_t)(H + j) * grow + (size_t)t * s4 + q];
    const f32x4 in_ = gi4[(size_t)(2 * H + j) * grow + (size_t)t * s4 + q];
    const f32x4 hr = gh4[(size_t)j * s4 + q], hz = gh4[(size_t)(H + j) * s4 + q], hn_ = gh4[(size_t)(2 * H + j) * s4 + q];
    f32x4* hs4 = (f32x4*)hs;
    const size_t hrow = (size_t)(T + 1) * s4;
    const f32x4 hp = hs4[(size_t)j * hrow + (size_t)t * s4 + q];
    f32x4 r, z, n, o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r[e] = 1.f / (1.f + expf(-(ir[e] + hr[e])));
        z[e] = 1.f / (1.f + expf(-(iz[e] + hz[e])));
        n[e] = tanhf(in_[e] + r[e] * hn_[e]);
        o[e] = (1.f - z[e]) * n[e] + z[e] * hp[e];
    }
    hs4[(size_t)j * hrow + (size_t)(t + 1) * s4 + q] = o;
    if (gates) {
        f32x4* g4 = (f32x4*)gates;
        const size_t plane = (size_t)H * T * s4;
        const size_t o_ = ((size_t)j * T + t) * s4 + q;
        g4[o_] = r; g4[plane + o_] = z; g4[2 * plane + o_] = n; g4[3 * plane + o_] = hn_;
    }
}

// time step t of the backward through time.  dh_t = dhs[:, t+1] (+ carry, the W_hh^T dgh of step t+1, when non-NULL):
//   dn = dh (1-z);  dnp = dn (1-n^2);  dzp = dh (h_{t-1} - n) z (1-z);  drp = dnp gh_n r (1-r)
//   dgi_all[:, t] = (drp, dzp, dnp);  dgh_all[:, t] = (drp, dzp, dnp r);  dhs[:, t] += dh z   (direct path to h_{t-1})
__global__ __launch_bounds__(256) void tgru_cell_bwd_kernel(float* dhs, const float* __restrict__ carry,
                                                            const float* __restrict__ hs, const float* __restrict__ gates,
                                                            float* __restrict__ dgi_all, float* __restrict__ dgh_all,
                                                            int H, int T, int t, int SP, int S) {
    const int s4 = SP / 4;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)H * s4) return;
    const int j = (int)(i / s4), q = (int)(i % s4);
    f32x4* dhs4 = (f32x4*)dhs;
    const size_t hrow = (size_t)(T + 1) * s4;
    f32x4 dh = dhs4[(size_t)j * hrow + (size_t)(t + 1) * s4 + q];
    if (carry) {
        const f32x4 cv = ((const f32x4*)carry)[(size_t)j * s4 + q];
#pragma unroll
        for (int e = 0; e < 4; ++e) dh[e] += cv[e];
    }
    const f32x4 hp = ((const f32x4*)hs)[(size_t)j * hrow + (size_t)t * s4 + q];
    const f32x4* g4 = (const f32x4*)gates;
    const size_t plane = (size_t)H * T * s4;
    const size_t o_ = ((size_t)j * T + t) * s4 + q;
    const f32x4 r = g4[o_], z = g4[plane + o_], n = g4[2 * plane + o_], ghn = g4[3 * plane + o_];
    f32x4 drp, dzp, dnp, dnr, dprev;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = (4 * q + e < S) ? dh[e] : 0.f;          // padded sequences carry no gradient
        const float dn = d * (1.f - z[e]);
        dnp[e] = dn * (1.f - n[e] * n[e]);
        dzp[e] = d * (hp[e] - n[e]) * z[e] * (1.f - z[e]);
        drp[e] = dnp[e] * ghn[e] * r[e] * (1.f - r[e]);
        dnr[e] = dnp[e] * r[e];
        dprev[e] = d * z[e];
    }
    f32x4* dgi4 = (f32x4*)dgi_all;
    f32x4* dgh4 = (f32x4*)dgh_all;
    const size_t grow = (size_t)T * s4;
    const size_t g0 = (size_t)j * grow + (size_t)t * s4 + q;
    dgi4[g0] = drp; dgi4[(size_t)H * grow + g0] = dzp; dgi4[(size_t)2 * H * grow + g0] = dnp;
    dgh4[g0] = drp; dgh4[(size_t)H * grow + g0] = dzp; dgh4[(size_t)2 * H * grow + g0] = dnr;
    f32x4 acc = dhs4[(size_t)j * hrow + (size_t)t * s4 + q];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += dprev[e];
    dhs4[(size_t)j * hrow + (size_t)t * s4 + q] = acc;
}

// ---------------------------------------------------------------- BatchNorm statistics -> affine
// (both finalize kernels leave the partial rows they consumed ZERO: a producer that is told so -- TRUNET_EPI_PREZERO /
// TRUNET_DG_PREZERO -- needs no zero-fill launch of its own for the rows its idle workgroups do not write)
__global__ __launch_bounds__(256) void bn_finalize_fwd_kernel(float* __restrict__ partials, int nparts, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, float momentum,
                                                              float* running_mean, float* running_var, float* scale,
                                                              float* shift, float* mean_o, float* rstd_o,
                                                              long long* num_batches_tracked) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int g = threadIdx.x; g < nparts; g += 256) {
        f32x2* pp = (f32x2*)(partials + ((size_t)g * C + c) * 2);
        const f32x2 v = *pp;
        a += (double)v[0];
        b += (double)v[1];
        *pp = f32x2{0.f, 0.f};
    }
    a = block_sum_f64(a, red);
    b = block_sum_f64(b, red);
    if (threadIdx.x == 0) {
        if (c == 0 && num_batches_tracked) *num_batches_tracked += 1;     // BatchNorm1d.num_batches_tracked (int64)
        double mean = a / count;
        double var = b / count - mean * mean;
        if (var < 0.0) var = 0.0;
        float rstd = (float)(1.0 / sqrt(var + (double)eps));
        float sc = gamma[c] * rstd;
        scale[c] = sc;
        shift[c] = beta[c] - (float)mean * sc;
        mean_o[c] = (float)mean;
        rstd_o[c] = rstd;
        if (running_mean) {
            double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
        }
    }
}

__global__ void bn_eval_affine_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv,
                                      float eps, float* scale, float* shift) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
}

__global__ __launch_bounds__(256) void bn_finalize_bwd_kernel(float* __restrict__ partials, int nparts, int C,
                                                              double count, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              float* dgamma, float* dbeta, float* ca, float* cb, float* cc) {
    __shared__ double red[256];
    const int c = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int g = threadIdx.x; g < nparts; g += 256) {
        f32x2* pp = (f32x2*)(partials + ((size_t)g * C + c) * 2);
        const f32x2 v = *pp;
        a += (double)v[0];
        b += (double)v[1];
        *pp = f32x2{0.f, 0.f};
    }
    a = block_sum_f64(a, red);   // sum dy
    b = block_sum_f64(b, red);   // sum dy*(z-mean)
    if (threadIdx.x == 0) {
        const double r = rstd[c], g = gamma[c], mu = mean[c];
        const double m1 = a / count;             // mean(dy)
        const double m2 = r * b / count;         // mean(dy*xhat)
        dgamma[c] = (float)(r * b);
        dbeta[c] = (float)a;
        ca[c] = (float)(g * r);
        cb[c] = (float)(-g * r * r * m2);
        cc[c] = (float)(-g * r * m1 + g * r * r * m2 * mu);
    }
}

// ---------------------------------------------------------------- optimizer
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd,
                             float bc1, float bc2_sqrt) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float gi = g[i];
    float pi = p[i] * (1.f - lr * wd);
    float mi = b1 * m[i] + (1.f - b1) * gi;
    float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - (lr / bc1) * (mi / denom);
}

// one block (the caller passes no scratch for a second stage): 1024 threads, 16-byte loads, four independent chains
__global__ __launch_bounds__(1024) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* out) {
    __shared__ double red[1024];
    const int tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int64_t n4 = ((reinterpret_cast<uintptr_t>(g) & 15) == 0) ? n / 4 : 0;
    const f32x4* g4 = (const f32x4*)g;
    for (int64_t i = tid; i < n4; i += 1024) {
        const f32x4 v = g4[i];
        s0 += (double)v[0] * (double)v[0];
        s1 += (double)v[1] * (double)v[1];
        s2 += (double)v[2] * (double)v[2];
        s3 += (double)v[3] * (double)v[3];
    }
    for (int64_t i = 4 * n4 + tid; i < n; i += 1024) s0 += (double)g[i] * (double)g[i];
    red[tid] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[0] = (float)red[0];
}

// 64-bit content checksum of a list of device buffers in ONE launch (blockIdx.y = buffer): every 32-bit word is mixed with
// its position and the buffer index and the results are summed (order-independent, so atomics are fine).  TRUNet.folded keys
// its cached eval artefact on it: weights written through `p.data` (util.weight_scaling_init of the reference) move no
// torch version counter.  `out` must be zero on entry.
struct ChecksumDesc { const uint32_t* ptr; long long nwords; };
__global__ __launch_bounds__(256) void checksum_batch_kernel(const ChecksumDesc* __restrict__ desc, unsigned long long* out) {
    __shared__ unsigned long long red[256];
    const ChecksumDesc d = desc[blockIdx.y];
    unsigned long long acc = 0ull;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < d.nwords; i += (long long)gridDim.x * 256) {
        unsigned long long h = (unsigned long long)d.ptr[i] + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1) +
                               0xC2B2AE3D27D4EB4Full * (unsigned long long)(blockIdx.y + 1);
        h ^= h >> 31; h *= 0x7FB5D329728EA185ull; h ^= h >> 27; h *= 0x81DADEF4BC2DD44Dull; h ^= h >> 33;
        acc += h;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(out, red[0]);
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_to_frames_last(const float* x, float* y, int N, int C, int L, int NP, void* stream) {
    if (!x || !y || N <= 0 || NP < N) return TRUNET_EINVAL;
    int R = C * L;
    hipLaunchKernelGGL(to_frames_last_kernel, dim3((NP + 31) / 32, (R + 31) / 32), dim3(32, 8), 0, ST, x, y, N, R, NP);
    return trunet_launch_status();
}

extern "C" int trunet_from_frames_last(const float* x, float* y, int N, int C, int L, int NP, void* stream) {
    if (!x || !y || N <= 0 || NP < N) return TRUNET_EINVAL;
    int R = C * L;
    hipLaunchKernelGGL(from_frames_last_kernel, dim3((NP + 31) / 32, (R + 31) / 32), dim3(32, 8), 0, ST, x, y, N, R, NP);
    return trunet_launch_status();
}

extern "C" int trunet_gru_cell(const float* gi, const float* gh, const float* h, float* h_new, int H, int L, int NP,
                               void* stream) {
    if (!gi || !gh || !h || !h_new || H <= 0 || L <= 0 || NP <= 0 || (NP % 4)) return TRUNET_EINVAL;
    const size_t R4 = (size_t)L * NP / 4;
    const size_t n = (size_t)H * R4;
    hipLaunchKernelGGL(gru_cell_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, gi, gh, h, h_new, H, R4);
    return trunet_launch_status();
}

extern "C" int trunet_to_seq_major(const float* x, float* y, const float* scale, const float* shift, int relu, int C,
                                   int Lf, int T, int B, int NP, int SP, void* stream) {
    if (!x || !y || C <= 0 || Lf <= 0 || T <= 0 || B <= 0 || (size_t)B * T > (size_t)NP || B * Lf > SP) return TRUNET_EINVAL;
    if (hipMemsetAsync(y, 0, (size_t)C * T * SP * sizeof(float), ST) != hipSuccess) return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(to_seq_major_kernel, dim3((T + 31) / 32, (B + 31) / 32, C * Lf), dim3(32, 8), 0, ST, x, y, scale,
                       shift, Lf, T, B, NP, SP, (scale && relu) ? 0.f : -3.0e38f);
    return trunet_launch_status();
}

extern "C" int trunet_from_seq_major_nparts(int Lf, int T, int B) { return ((T + 31) / 32) * ((B + 31) / 32) * Lf; }

extern "C" int trunet_from_seq_major(const float* y, float* x, const float* zsrc, const float* scale, const float* shift,
                                     const float* mean, float* partials, int C, int Lf, int T, int B, int NP, int SP,
                                     void* stream) {
    if (!x || !y || C <= 0 || Lf <= 0 || T <= 0 || B <= 0 || (size_t)B * T > (size_t)NP || B * Lf > SP) return TRUNET_EINVAL;
    if (zsrc && (!scale || !shift || !mean || !partials)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(from_seq_major_kernel, dim3((T + 31) / 32, (B + 31) / 32, C * Lf), dim3(32, 8), 0, ST, y, x, zsrc,
                       scale, shift, mean, partials, C, Lf, T, B, NP, SP);
    return trunet_launch_status();
}

extern "C" int trunet_tgru_cell_fwd(const float* gi_all, const float* gh, float* hs, float* gates, int H, int T, int t,
                                    int SP, void* stream) {
    if (!gi_all || !gh || !hs || H <= 0 || T <= 0 || t < 0 || t >= T || SP <= 0 || (SP % 4)) return TRUNET_EINVAL;
    const size_t n = (size_t)H * (SP / 4);
    hipLaunchKernelGGL(tgru_cell_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, gi_all, gh, hs, gates, H,
                       T, t, SP);
    return trunet_launch_status();
}

extern "C" int trunet_tgru_cell_bwd(float* dhs, const float* carry, const float* hs, const float* gates, float* dgi_all,
                                    float* dgh_all, int H, int T, int t, int SP, int S, void* stream) {
    if (!dhs || !hs || !gates || !dgi_all || !dgh_all || H <= 0 || T <= 0 || t < 0 || t >= T || SP <= 0 || (SP % 4))
        return TRUNET_EINVAL;
    const size_t n = (size_t)H * (SP / 4);
    hipLaunchKernelGGL(tgru_cell_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, dhs, carry, hs, gates,
                       dgi_all, dgh_all, H, T, t, SP, S);
    return trunet_launch_status();
}

extern "C" int trunet_from_frames_last_affine(const float* x, float* y, int N, int C, int L, int NP, const float* scale,
                                              const float* shift, int relu, void* stream) {
    if (!x || !y || !scale || !shift || N <= 0 || NP < N || C <= 0 || L <= 0) return TRUNET_EINVAL;
    int R = C * L;
    hipLaunchKernelGGL(from_frames_last_affine_kernel, dim3((NP + 31) / 32, (R + 31) / 32), dim3(32, 8), 0, ST, x, y, N, R,
                       NP, L, scale, shift, relu ? 0.f : -3.0e38f);
    return trunet_launch_status();
}

extern "C" int trunet_conv_first_fwd(const float* x, const float* w, const float* b, float* y, int Cin, int Cout, int K,
                                     int S, int Lin, int Lout, int NP, void* stream) {
    if (!x || !w || !b || !y || Cout <= 0 || S <= 0 || Lin <= 0 || Lout <= 0 || NP <= 0 || (NP % 128)) return TRUNET_EINVAL;
    dim3 grid(NP / 128, (Lout + 7) / 8), block(32, 8);
    if (K == 5 && Cin == 3) hipLaunchKernelGGL((conv_first_kernel<3, 5>), grid, block, 0, ST, x, w, b, y, Cout, S, Lin, Lout, NP);
    else if (K == 5 && Cin == 4) hipLaunchKernelGGL((conv_first_kernel<4, 5>), grid, block, 0, ST, x, w, b, y, Cout, S, Lin, Lout, NP);
    else return TRUNET_ENOTSUP;
    return trunet_launch_status();
}

extern "C" int trunet_relu_bwd_stats_nparts(void) { return DW_PARTS; }

extern "C" int trunet_relu_bwd_stats(float* dy, const float* z, const float* scale, const float* shift, const float* mean,
                                     float* partials, int C, int L, int NP, int N, void* stream) {
    if (!dy || !z || C <= 0 || L <= 0 || N <= 0 || NP < N || (NP % 128)) return TRUNET_EINVAL;
    if ((scale == nullptr) != (shift == nullptr) || (mean != nullptr) != (partials != nullptr)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(relu_bwd_stats_kernel, dim3(DW_PARTS, C), dim3(256), 0, ST, dy, z, scale, shift, mean, partials, C,
                       L, NP, N);
    return trunet_launch_status();
}

extern "C" int trunet_bn_finalize_fwd(float* partials, int nparts, int C, double count, const float* gamma,
                                      const float* beta, float eps, float momentum, float* running_mean,
                                      float* running_var, float* scale, float* shift, float* mean, float* rstd,
                                      int64_t* num_batches_tracked, void* stream) {
    if (!partials || !gamma || !beta || !scale || !shift || !mean || !rstd || C <= 0 || nparts <= 0) return TRUNET_EINVAL;
    if (!(count > 0.0)) return TRUNET_EINVAL;          // count <= 0 (or NaN) would write NaN scales
    if ((running_mean == nullptr) != (running_var == nullptr)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(bn_finalize_fwd_kernel, dim3(C), dim3(256), 0, ST, partials, nparts, C, count, gamma, beta, eps,
                       momentum, running_mean, running_var, scale, shift, mean, rstd, (long long*)num_batches_tracked);
    return trunet_launch_status();
}

extern "C" int trunet_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                                     const float* running_var, float eps, float* scale, float* shift, void* stream) {
    if (!gamma || !beta || !running_mean || !running_var || !scale || !shift || C <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(bn_eval_affine_kernel, dim3((C + 127) / 128), dim3(128), 0, ST, C, gamma, beta, running_mean,
                       running_var, eps, scale, shift);
    return trunet_launch_status();
}

extern "C" int trunet_bn_finalize_bwd(float* partials, int nparts, int C, double count, const float* gamma,
                                      const float* mean, const float* rstd, float* dgamma, float* dbeta, float* ca,
                                      float* cb, float* cc, void* stream) {
    if (!partials || !gamma || !mean || !rstd || !dgamma || !dbeta || !ca || !cb || !cc) return TRUNET_EINVAL;
    if (C <= 0 || nparts <= 0 || !(count > 0.0)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(bn_finalize_bwd_kernel, dim3(C), dim3(256), 0, ST, partials, nparts, C, count, gamma, mean, rstd,
                       dgamma, dbeta, ca, cb, cc);
    return trunet_launch_status();
}

extern "C" int trunet_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                            float eps, float wd, int step, void* stream) {
    if (!p || !g || !m || !v || n <= 0 || step < 1) return TRUNET_EINVAL;
    float bc1 = 1.f - powf(beta1, (float)step);
    float bc2s = sqrtf(1.f - powf(beta2, (float)step));
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, p, g, m, v, n, lr, beta1, beta2,
                       eps, wd, bc1, bc2s);
    return trunet_launch_status();
}

extern "C" int trunet_checksum_batch(const void* desc, int n, uint64_t* out, void* stream) {
    if (!desc || !out || n <= 0 || n > 65535) return TRUNET_EINVAL;
    hipLaunchKernelGGL(checksum_batch_kernel, dim3(8, n), dim3(256), 0, ST, (const ChecksumDesc*)desc, (unsigned long long*)out);
    return trunet_launch_status();
}

extern "C" int trunet_sumsq(const float* g, int64_t n, float* out, void* stream) {
    if (!g || !out || n <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(sumsq_kernel, dim3(1), dim3(1024), 0, ST, g, n, out);
    return trunet_launch_status();
}

// ---------------------------------------------------------------- calibration (bench/diagnostics only)
namespace {
__global__ __launch_bounds__(256) void mfma_peak_kernel(float* out, int iters, float seed) {
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    float a = seed + threadIdx.x * 1e-3f, b = seed * 0.5f + threadIdx.x * 2e-3f;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[t][r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
}  // namespace

/* Sustained fp32 MFMA rate of this device at its operating clock: launches `blocks` x 256 threads, each wave
 * issuing 16*iters v_mfma_f32_32x32x2_f32 on 4 independent accumulators.  flops = blocks*4*16*iters*4096. */
extern "C" int trunet_debug_mfma_peak(float* out, int blocks, int iters, void* stream) {
    if (!out || blocks <= 0 || iters <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(256), 0, ST, out, iters, 1.0f);
    return trunet_launch_status();
}
