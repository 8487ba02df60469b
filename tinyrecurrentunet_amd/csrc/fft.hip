// FFT-based stages of the hot path, one LDS Stockham radix-2 FFT per workgroup (256 threads):
//   * STFT features  (dataset.py:246-272): rect-window rFFT-512 -> (norm-dB-mag, [PCEN], sin, cos)
//   * PCEN           (dataset.py:56-76)
//   * mask + iSTFT   (phm.py:31-45 + R5, dataset.py:182-203,275-298): net output -> audio, and its backward
//   * L1 loss        (util.py:239-240)
//   * multi-resolution STFT loss (stft_loss.py:9-166), forward sums and backward
// Two real sequences share one complex FFT (z = a + j b;  A[k] = (Z[k] + conj Z[N-k])/2,
// B[k] = (Z[k] - conj Z[N-k])/(2j)): two STFT frames per transform in the feature / iSTFT kernels,
// the (predicted, target) pair of one frame in the loss kernels.  All of these stages are HBM-bound.
#include "common.hpp"
#include "fft_common.hpp"

namespace {

// In-LDS Stockham autosort FFT of size n = 2^logn by all 256 threads of the block.
// tw[t] = exp(-2*pi*i*t/n), t < n/2.  inverse => conjugated twiddles (unnormalised).
// Returns the buffer (a or b) that holds the natural-order result.  Ends with a barrier.
__device__ cpx* fft_lds(cpx* a, cpx* b, int n, int logn, const cpx* __restrict__ tw, bool inverse) {
    // Stockham autosort, radix 4 (one radix-2 stage first when log2 n is odd): 5 / 5 / 6 barriers for n = 512 / 1024 / 2048
    // instead of 9 / 10 / 11, and half the LDS traffic
    const int half = n >> 1, quarter = n >> 2;
    cpx* x = a;
    cpx* y = b;
    int ns = 1;
    int s = 0;
    if (logn & 1) {
        __syncthreads();
        for (int j = threadIdx.x; j < half; j += blockDim.x) {
            const cpx u = x[j], v = x[j + half];
            y[2 * j] = make_float2(u.x + v.x, u.y + v.y);
            y[2 * j + 1] = make_float2(u.x - v.x, u.y - v.y);
        }
        cpx* t = x; x = y; y = t;
        ns = 2;
        s = 1;
    }
    for (; s < logn; s += 2) {
        __syncthreads();
        const int tstep = quarter / ns;          // twiddle index step: exp(-2 pi i k / (4 ns)) = tw[k * n / (4 ns)]
        for (int j = threadIdx.x; j < quarter; j += blockDim.x) {
            const int k = j & (ns - 1);
            const int t1 = k * tstep;
            cpx w1 = tw[t1], w2 = tw[2 * t1];
            const int t3 = 3 * t1;
            cpx w3 = tw[t3 >= half ? t3 - half : t3];
            if (t3 >= half) { w3.x = -w3.x; w3.y = -w3.y; }
            if (inverse) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
            const cpx u0 = x[j];
            const cpx u1 = cmul(w1, x[j + quarter]);
            const cpx u2 = cmul(w2, x[j + 2 * quarter]);
            const cpx u3 = cmul(w3, x[j + 3 * quarter]);
            const cpx v0 = make_float2(u0.x + u2.x, u0.y + u2.y);
            const cpx v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
            const cpx v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
            const cpx d = make_float2(u1.x - u3.x, u1.y - u3.y);
            // forward: (-i) d = (d.y, -d.x); inverse: (+i) d = (-d.y, d.x)
            const cpx v3 = inverse ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);
            const int j0 = ((j - k) << 2) + k;
            y[j0] = make_float2(v0.x + v2.x, v0.y + v2.y);
            y[j0 + ns] = make_float2(v1.x + v3.x, v1.y + v3.y);
            y[j0 + 2 * ns] = make_float2(v0.x - v2.x, v0.y - v2.y);
            y[j0 + 3 * ns] = make_float2(v1.x - v3.x, v1.y - v3.y);
        }
        cpx* t = x; x = y; y = t;
        ns <<= 2;
    }
    __syncthreads();
    return x;
}

// NI = n / 256 of the STFT-loss kernels -> log2 n (NI = 2, 4, 8); NI = 0: the runtime-sized form
template <int NI, bool INV>
__device__ __forceinline__ cpx* fft_lds_ni(cpx* a, cpx* b, int n, int logn, const cpx* __restrict__ tw) {
    if constexpr (NI == 2) return fft_lds_t<9, INV>(a, b, tw);
    else if constexpr (NI == 4) return fft_lds_t<10, INV>(a, b, tw);
    else if constexpr (NI == 8) return fft_lds_t<11, INV>(a, b, tw);
    else return fft_lds(a, b, n, logn, tw, INV);
}

__device__ __forceinline__ int reflect_idx(int j, int L) {
    if (j < 0) j = -j;
    if (j >= L) j = 2 * (L - 1) - j;
    return j;
}

constexpr int NF = 512;      // feature STFT size (dataset.py:133)
constexpr int HOPF = 128;    // dataset.py:134
constexpr int BINS = 257;

// ---------------------------------------------------------------- STFT features
// one bin of dataset.py:246-272 (amp_to_db :207-211, norm :229-235, sin / cos of the phase) -> magnitude
__device__ __forceinline__ float spectral_features(float re, float im, float& nm, float& sn, float& cs) {
    const float mag = sqrtf(re * re + im * im);
    const float db = 20.f * log10f(fmaxf(mag, 1e-7f)) - 25.f;
    nm = ((db + 100.f) / 100.f) * 2.f - 1.f;
    nm = fminf(fmaxf(nm, -1.f), 1.f);
    sn = 0.f; cs = 1.f;             // angle(0) = 0
    if (mag > 0.f) { sn = im / mag; cs = re / mag; }
    return mag;
}

// frames t0, t0 + 1 of utterance x (L samples, centred, reflect padding) as ONE complex sequence; a frame past T is zero
__device__ __forceinline__ cpx load_audio_pair(const float* __restrict__ x, int t0, int T, int L, int i) {
    const float va = x[reflect_idx(t0 * HOPF + i - NF / 2, L)];
    const float vb = (t0 + 1 < T) ? x[reflect_idx((t0 + 1) * HOPF + i - NF / 2, L)] : 0.f;
    return make_float2(va, vb);
}

// The fp32 transform of a real sequence is Hermitian only to rounding, so split_pair leaves in each frame an error proportional
// to its PARTNER's norm.  Next to a loud frame an all-zero one (digital silence before an onset, a muted stream beside a talking
// one) would get |X| ~ 1e-7 ||partner|| where the reference has exactly 0, which PCEN (eps 1e-6) turns into values as large as
// those of speech, and noise for (sin, cos) where the reference has (0, 1).  So a frame whose 512 staged samples are all exactly
// zero gets an exactly zero spectrum: every wave notes which real halves it staged a non-zero sample into (bit 0: real, bit 1:
// imaginary) in its own LDS word, the transform's first barrier publishes the four words, silence_pair reads them after the
// split.  No barrier of its own; the same in every kernel that pairs two frames, so their bit-for-bit promises hold.
__device__ __forceinline__ void note_live(int* wl, cpx v0, cpx v1) {
    const int re = __any(v0.x != 0.f || v1.x != 0.f), im = __any(v0.y != 0.f || v1.y != 0.f);
    if ((threadIdx.x & 63) == 0) wl[threadIdx.x >> 6] = (re ? 1 : 0) | (im ? 2 : 0);
}
__device__ __forceinline__ int pair_live(const int* wl) { return wl[0] | wl[1] | wl[2] | wl[3]; }
__device__ __forceinline__ void silence_pair(int live, cpx& A, cpx& B) {
    if (!(live & 1)) A = make_float2(0.f, 0.f);
    if (!(live & 2)) B = make_float2(0.f, 0.f);
    // The arithmetic behind this must stay the arithmetic of a plain split_pair: with the selects in sight the compiler
    // contracts sqrtf(re * re + im * im) and the smoother differently from kernel to kernel (fma(re, re, im * im) here,
    // fma(im, im, re * re) there: the dense and the frames-last kernels were one ulp apart), which ends the bit-for-bit
    // promises between the entry points.  Opaque registers keep every kernel on the contraction it had.
    asm volatile("" : "+v"(A.x), "+v"(A.y), "+v"(B.x), "+v"(B.y));
}

// thread i stages samples i and i + 256 (256 threads)
__device__ __forceinline__ void stage_pair(cpx* sa, int* wl, cpx v0, cpx v1) {
    sa[threadIdx.x] = v0;
    sa[threadIdx.x + 256] = v1;
    note_live(wl, v0, v1);
}

__device__ __forceinline__ void stage_audio_pair(cpx* sa, int* wl, const float* __restrict__ x, int t0, int T, int L) {
    stage_pair(sa, wl, load_audio_pair(x, t0, T, L, (int)threadIdx.x), load_audio_pair(x, t0, T, L, (int)threadIdx.x + 256));
}

// grid (ceil(T/2), B); feat: (B*T, C, 257); mag (optional): (B, T, 257)
__global__ __launch_bounds__(256) void stft_features_kernel(const float* __restrict__ audio, float* __restrict__ feat,
                                                            float* __restrict__ mag_out, const cpx* __restrict__ tw,
                                                            int L, int T, int C) {
    __shared__ cpx sa[NF], sb[NF];
    __shared__ int wl[4];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * 2;
    stage_audio_pair(sa, wl, audio + (size_t)b * L, t0, T, L);
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    const int live = pair_live(wl);
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
        split_pair(Z, k, NF, X[0], X[1]);
        silence_pair(live, X[0], X[1]);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int t = t0 + f;
            if (t >= T) continue;
            float nm, sn, cs;
            const float mag = spectral_features(X[f].x, X[f].y, nm, sn, cs);
            float* o = feat + ((size_t)(b * T + t) * C) * BINS + k;
            o[0] = nm;
            o[(size_t)(C - 2) * BINS] = sn;
            o[(size_t)(C - 1) * BINS] = cs;
            if (mag_out) mag_out[((size_t)b * T + t) * BINS + k] = mag;
        }
    }
}

// PCEN (dataset.py:56-76): M[0] = s x[0]; M[t] = (1-s) M[t-1] + s x[t]; (x/(M+eps)^alpha + delta)^r - delta^r
// Two launches.  pcen_scan_kernel: block = (utterance b, 64 bins); the smoother M is a cheap sequential scan over T (one
// wave, from LDS chunks that all four waves load) and is written into the OUTPUT slots.  pcen_pow_kernel: the three powf
// per element are not part of the recurrence: one thread per (b, t, bin) replaces M by the result in place.
constexpr int PCEN_TC = 256;
__global__ __launch_bounds__(256) void pcen_scan_kernel(const float* __restrict__ mag, float* __restrict__ out, int T,
                                                        int out_stride, float s) {
    __shared__ float xs[PCEN_TC][64];
    const int tid = threadIdx.x;
    const int kb = blockIdx.x * 64;
    const int b = blockIdx.y;
    const float* x = mag + (size_t)b * T * BINS;
    float* o = out + (size_t)b * T * out_stride;
    float M = 0.f;                          // carried by threads 0..63 (bin kb + tid)
    for (int t0 = 0; t0 < T; t0 += PCEN_TC) {
        const int tc = min(PCEN_TC, T - t0);
        for (int i = tid; i < tc * 64; i += 256) {
            const int t = i >> 6, k = i & 63;
            xs[t][k] = (kb + k < BINS) ? x[(size_t)(t0 + t) * BINS + kb + k] : 0.f;
        }
        __syncthreads();
        if (tid < 64) {
            for (int t = 0; t < tc; ++t) {
                const float v = xs[t][tid];
                M = (t0 + t == 0) ? s * v : (1.f - s) * M + s * v;
                xs[t][tid] = M;
            }
        }
        __syncthreads();
        for (int i = tid; i < tc * 64; i += 256) {
            const int t = i >> 6, k = i & 63;
            if (kb + k < BINS) o[(size_t)(t0 + t) * out_stride + kb + k] = xs[t][k];
        }
        __syncthreads();
    }
}

// (x / (M + eps)^alpha + delta)^r - delta^r  (dataset.py:70-75), shared by the offline and the streaming front end.  libm's powf on
// purpose: the two powers through v_exp_f32 / v_log_f32 (and a square root for r = 0.5) were built in round 4 -- 0.135 -> ~0.06 ms
// per step, features within 2e-6 -- and taken out again: a 1e-6 change of the network INPUT moves the full-size gradients as far
// as any other change of the forward rounding does (test_cfg2_full_size_train_step_vs_oracle: 8.6e-4 -> 2.1e-2 against the
// oracle at the gated seed), and the features are pinned to the reference's torch.pow.
__device__ __forceinline__ float pcen_value(float v, float M, float eps, float alpha, float delta, float r, float dr) {
    return powf(v / powf(M + eps, alpha) + delta, r) - dr;
}

__global__ __launch_bounds__(256) void pcen_pow_kernel(const float* __restrict__ mag, float* __restrict__ out, int rows,
                                                       int out_stride, float eps, float alpha, float delta, float r,
                                                       float dr) {
    const int k = blockIdx.x * 256 + threadIdx.x;      // bin
    const int row = blockIdx.y;                        // b*T + t
    if (k >= BINS || row >= rows) return;
    const float v = mag[(size_t)row * BINS + k];
    float* o = out + (size_t)row * out_stride + k;
    const float M = *o;
    *o = pcen_value(v, M, eps, alpha, delta, r, dr);
}

// ---------------------------------------------------------------- mask + iSTFT
// Per bin of the net output o (8 channels, R7): A = 10^(2.5 (clamp(o0)+1) - 3.75);
// phi_m = atan2(o2, o3); phi_n = atan2(o6, o7); M = sigmoid(beta (phi_m - phi_n)) A; X = M e^{j phi_m}.
struct MaskVals { float A, S, cm, sm, r2m, r2n, c0; };

__device__ __forceinline__ MaskVals mask_vals(const float* o, size_t cs, float beta) {
    MaskVals v;
    const float c0 = o[0], c2 = o[2 * cs], c3 = o[3 * cs], c6 = o[6 * cs], c7 = o[7 * cs];
    v.c0 = c0;
    const float cc = fminf(fmaxf(c0, -1.f), 1.f);
    v.A = exp10f(2.5f * (cc + 1.f) - 3.75f);
    v.r2m = c2 * c2 + c3 * c3;
    v.r2n = c6 * c6 + c7 * c7;
    const float pm = atan2f(c2, c3), pn = atan2f(c6, c7);
    v.S = 1.f / (1.f + expf(-beta * (pm - pn)));
    if (v.r2m > 0.f) { const float ir = rsqrtf(v.r2m); v.cm = c3 * ir; v.sm = c2 * ir; }
    else { v.cm = 1.f; v.sm = 0.f; }
    return v;
}

// masked spectrum X = M e^{j phi_m} of bin k from the 8 channels at o (channel stride cs); a frame that does not exist
// (`valid` false: o is not read) is zero
__device__ __forceinline__ cpx masked_bin(const float* o, size_t cs, int k, bool valid, float beta) {
    cpx X = make_float2(0.f, 0.f);
    if (valid) {
        const MaskVals v = mask_vals(o, cs, beta);
        const float M = v.S * v.A;
        X = make_float2(M * v.cm, M * v.sm);
    }
    if (k == 0 || k == NF / 2) X.y = 0.f;     // c2r ignores the imaginary part of DC / Nyquist
    return X;
}

// bin k of two half spectra as one complex sequence: Z = Xa_full + j Xb_full (Hermitian extensions)
__device__ __forceinline__ void pack_pair(cpx* sa, int k, cpx Xa, cpx Xb) {
    sa[k] = make_float2(Xa.x - Xb.y, Xa.y + Xb.x);
    if (k > 0 && k < NF / 2) sa[NF - k] = make_float2(Xa.x + Xb.y, -Xa.y + Xb.x);
}

// grid (ceil(T/2), B); out_net: (B*T, 8, 257); frames: (B, T, 512) time-domain frames (irfft, 1/512)
__global__ __launch_bounds__(256) void mask_istft_frames_kernel(const float* __restrict__ net_out,
                                                                float* __restrict__ frames, const cpx* __restrict__ tw,
                                                                int T, float beta) {
    __shared__ cpx sa[NF], sb[NF];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * 2;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int t = t0 + f;
            X[f] = masked_bin(net_out + (size_t)(b * T + t) * 8 * BINS + k, BINS, k, t < T, beta);
        }
        pack_pair(sa, k, X[0], X[1]);
    }
    const cpx* z = fft_lds_t<9, true>(sa, sb, tw);
    for (int i = threadIdx.x; i < NF; i += 256) {
        const cpx v = z[i];
        frames[((size_t)b * T + t0) * NF + i] = v.x * (1.f / NF);
        if (t0 + 1 < T) frames[((size_t)b * T + t0 + 1) * NF + i] = v.y * (1.f / NF);
    }
}

__device__ __forceinline__ float ola_env(int p, int T) {
    // number of rectangular frames covering padded position p (window envelope of torch.istft)
    int hi = p / HOPF;
    if (hi > T - 1) hi = T - 1;
    int lo = (p - NF + HOPF) / HOPF;      // ceil((p - 511)/128) for p >= 0
    if (p - NF + 1 <= 0) lo = 0;
    return (float)(hi - lo + 1);
}

// audio[b][j] = sum_t frames[b][t][j + 256 - 128 t] / env ; optional L1 partial sums vs clean
__global__ __launch_bounds__(256) void ola_kernel(const float* __restrict__ frames, float* __restrict__ audio,
                                                  const float* __restrict__ clean, float* __restrict__ l1_partials,
                                                  int T, int L) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    float ad = 0.f;
    if (j < L) {
        const int p = j + NF / 2;
        int hi = p / HOPF; if (hi > T - 1) hi = T - 1;
        int lo = (p - NF + HOPF) / HOPF; if (p - NF + 1 <= 0) lo = 0;
        float s = 0.f;
        for (int t = lo; t <= hi; ++t) s += frames[((size_t)b * T + t) * NF + (p - t * HOPF)];
        s /= (float)(hi - lo + 1);
        audio[(size_t)b * L + j] = s;
        if (clean) ad = fabsf(s - clean[(size_t)b * L + j]);
    }
    if (l1_partials) {
        double r = block_sum_f64((double)ad, red);
        if (threadIdx.x == 0) l1_partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (float)r;
    }
}

// g_audio[i] = scale[0] * sign(den - clean)   (gradient of mean |den - clean|, scale = upstream/(B L))
__global__ void l1_grad_kernel(const float* __restrict__ den, const float* __restrict__ clean,
                               const float* __restrict__ scale, float* __restrict__ g, int64_t n) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float d = den[i] - clean[i];
    g[i] = (d > 0.f) ? scale[0] : ((d < 0.f) ? -scale[0] : 0.f);
}

// the windowed cotangent of frames t0, t0 + 1 of one utterance (g: its L samples of d loss / d audio) as ONE complex sequence
__device__ __forceinline__ cpx load_grad_pair(const float* __restrict__ g, int t0, int T, int L, int i) {
    float v[2] = {0.f, 0.f};
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int t = t0 + f;
        const int p = t * HOPF + i;
        const int j = p - NF / 2;
        if (t < T && j >= 0 && j < L) v[f] = g[j] / ola_env(p, T);
    }
    return make_float2(v[0], v[1]);
}

__device__ __forceinline__ void stage_grad_pair(cpx* sa, const float* __restrict__ g, int t0, int T, int L) {
    for (int i = threadIdx.x; i < NF; i += 256) sa[i] = load_grad_pair(g, t0, T, L, i);
}

// bin k of one frame: G = its bin of the transformed cotangent, o = the 8 net-output channels, g = their gradients
// (both with channel stride cs)
__device__ __forceinline__ void mask_bwd_bin(const float* __restrict__ o, float* __restrict__ g, size_t cs, cpx G, int k,
                                             float beta) {
    const float wk = (k == 0 || k == NF / 2) ? (1.f / NF) : (2.f / NF);
    const MaskVals v = mask_vals(o, cs, beta);
    const float dRe = wk * G.x;
    const float dIm = (k == 0 || k == NF / 2) ? 0.f : wk * G.y;
    const float M = v.S * v.A;
    const float dM = dRe * v.cm + dIm * v.sm;
    float dpm = M * (dIm * v.cm - dRe * v.sm);
    const float du = dM * v.A * v.S * (1.f - v.S);
    dpm += beta * du;
    const float dpn = -beta * du;
    const float dA = dM * v.S;
    const float dc0 = (v.c0 >= -1.f && v.c0 <= 1.f) ? dA * v.A * 2.5f * 2.302585092994046f : 0.f;
    const float c2 = o[2 * cs], c3 = o[3 * cs], c6 = o[6 * cs], c7 = o[7 * cs];
    g[0] = dc0;
    g[1 * cs] = 0.f;
    g[2 * cs] = (v.r2m > 0.f) ? dpm * c3 / v.r2m : 0.f;
    g[3 * cs] = (v.r2m > 0.f) ? -dpm * c2 / v.r2m : 0.f;
    g[4 * cs] = 0.f;
    g[5 * cs] = 0.f;
    g[6 * cs] = (v.r2n > 0.f) ? dpn * c7 / v.r2n : 0.f;
    g[7 * cs] = (v.r2n > 0.f) ? -dpn * c6 / v.r2n : 0.f;
}

// backward of mask + iSTFT: g_audio (B, L) -> g_net (B*T, 8, 257)
__global__ __launch_bounds__(256) void mask_istft_bwd_kernel(const float* __restrict__ g_audio,
                                                             const float* __restrict__ net_out,
                                                             float* __restrict__ g_net, const cpx* __restrict__ tw,
                                                             int T, int L, float beta) {
    __shared__ cpx sa[NF], sb[NF];
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * 2;
    stage_grad_pair(sa, g_audio + (size_t)b * L, t0, T, L);
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx G[2];
        split_pair(Z, k, NF, G[0], G[1]);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int t = t0 + f;
            if (t >= T) continue;
            const size_t base = (size_t)(b * T + t) * 8 * BINS + k;
            mask_bwd_bin(net_out + base, g_net + base, BINS, G[f], k, beta);
        }
    }
}

// ---------------------------------------------------------------- frames-last boundary
// The same three stages against the network's own layout [C][257][NP], frame n = b T + t in the last dimension (columns
// n >= N are padding), so that no transpose pass stands between them and the layer kernels.  A workgroup covers FLG consecutive
// frames, utterance boundaries or not, and goes through LDS (sx: one complex value per frame and bin), so that every global
// access to a frames-last row is FLG contiguous floats.  The transforms are the ones above, pair for pair: frames (t0 even,
// t0 + 1) of one utterance share a transform, the last frame of an odd T has a zero partner.  A pair that straddles a group's
// edge is transformed by both neighbours, each keeping its own frame.
constexpr int FLG = 32;

struct FlPair { int b, t0, next; };       // utterance, first frame of the pair, the first frame n after the pair

__device__ __forceinline__ FlPair fl_pair(int n, int T) {
    FlPair p;
    p.b = n / T;
    p.t0 = (n - p.b * T) & ~1;
    p.next = p.b * T + min(p.t0 + 2, T);
    return p;
}

// body(b, t0, slot, v0, v1) for every pair that holds one of the frames n0 .. min(n0 + FLG, N) - 1; slot = b T + t0 - n0 in
// [-1, FLG).  v0, v1 = load(b, t0, i) for i = threadIdx.x and threadIdx.x + 256: what this thread stages of the pair from
// global memory, requested one pair ahead, so that the round trip runs behind the previous pair's transform (a workgroup
// makes up to 17 transforms one after the other, and its LDS leaves room for only two workgroups per CU to hide it).
// The body stages into sa: fft_lds_t<9, .> leaves its result in sb and ends with a barrier, so sa is free by then, and a
// body needs no barrier of its own before the next pair is staged.
template <class Load, class Body>
__device__ __forceinline__ void fl_each_pair(int n0, int N, int T, Load load, Body body) {
    const int n1 = min(n0 + FLG, N);
    if (n0 >= n1) return;
    FlPair p = fl_pair(n0, T);
    cpx v0 = load(p.b, p.t0, (int)threadIdx.x), v1 = load(p.b, p.t0, (int)threadIdx.x + 256);
    for (;;) {
        const FlPair cur = p;
        const cpx c0 = v0, c1 = v1;
        const bool more = cur.next < n1;
        if (more) {
            p = fl_pair(cur.next, T);
            v0 = load(p.b, p.t0, (int)threadIdx.x);
            v1 = load(p.b, p.t0, (int)threadIdx.x + 256);
        }
        body(cur.b, cur.t0, cur.b * T + cur.t0 - n0, c0, c1);
        if (!more) break;
    }
}

// The transforms of a workgroup run one after the other, so they take their twiddles from LDS: a global (L1) round trip in
// every radix-4 stage, which eight workgroups per CU hide in the kernels above, would be paid 4 x 17 times in a row here, and
// its vmcnt wait would end the flight of the next pair's samples as well.  (fft_lds_t begins with a barrier.)
__device__ __forceinline__ void fl_stage_twiddles(cpx* stw, const cpx* __restrict__ tw) {
    if (threadIdx.x < NF / 2) stw[threadIdx.x] = tw[threadIdx.x];
}

// grid NP / FLG; x: [C][257][NP] (channel 1 of C = 4 is left for the PCEN kernels), mag (optional): [257][NP]; columns
// n >= N of the channels written here are zero
__global__ __launch_bounds__(256) void stft_features_fl_kernel(const float* __restrict__ audio, float* __restrict__ x,
                                                               float* __restrict__ mag_out, const cpx* __restrict__ tw,
                                                               int L, int T, int C, int N, int NP) {
    __shared__ cpx sa[NF], sb[NF], stw[NF / 2];
    __shared__ cpx sx[FLG][BINS];
    __shared__ int wl[2][4];                   // by the parity of the pair: a wave may stage the next pair while another still reads
    const int n0 = blockIdx.x * FLG;
    int par = 0;
    fl_stage_twiddles(stw, tw);
    fl_each_pair(n0, N, T,
                 [&](int b, int t0, int i) { return load_audio_pair(audio + (size_t)b * L, t0, T, L, i); },
                 [&](int b, int t0, int slot, cpx v0, cpx v1) {
        stage_pair(sa, wl[par], v0, v1);
        const cpx* Z = fft_lds_t<9, false>(sa, sb, stw);
        const int live = pair_live(wl[par]);
        par ^= 1;
        for (int k = threadIdx.x; k < BINS; k += 256) {
            cpx X[2];
            split_pair(Z, k, NF, X[0], X[1]);
            silence_pair(live, X[0], X[1]);
#pragma unroll
            for (int f = 0; f < 2; ++f)
                if (t0 + f < T && slot + f >= 0 && slot + f < FLG) sx[slot + f][k] = X[f];
        }
        if (Z != sb) __syncthreads();          // (folds away: the result lies in sb, and the transform is done with sa)
    });
    __syncthreads();
    const int fn = threadIdx.x & (FLG - 1);
    const int n = n0 + fn;
    const size_t plane = (size_t)BINS * NP;
#pragma unroll 4
    for (int k = threadIdx.x / FLG; k < BINS; k += 256 / FLG) {
        float nm = 0.f, sn = 0.f, cs = 0.f, mag = 0.f;
        if (n < N) {
            const cpx X = sx[fn][k];
            mag = spectral_features(X.x, X.y, nm, sn, cs);
        }
        float* o = x + (size_t)k * NP + n;
        o[0] = nm;
        o[(size_t)(C - 2) * plane] = sn;
        o[(size_t)(C - 1) * plane] = cs;
        if (mag_out) mag_out[(size_t)k * NP + n] = mag;
    }
}

// pcen_scan_kernel on mag [257][NP]: a row is contiguous in t, so the chunk is loaded along t and transposed in LDS (the
// scan reads xs[t][bin]; 65 columns keep both directions free of bank conflicts).  out: channel 1 of x, [257][NP].
constexpr int PCEN_FL_TC = 128;
__global__ __launch_bounds__(256) void pcen_scan_fl_kernel(const float* __restrict__ mag, float* __restrict__ out, int T,
                                                           int NP, float s) {
    __shared__ float xs[PCEN_FL_TC][65];
    const int tid = threadIdx.x;
    const int kb = blockIdx.x * 64;
    const size_t col0 = (size_t)blockIdx.y * T;
    float M = 0.f;                          // carried by threads 0..63 (bin kb + tid)
    for (int t0 = 0; t0 < T; t0 += PCEN_FL_TC) {
        const int tc = min(PCEN_FL_TC, T - t0);
        for (int i = tid; i < PCEN_FL_TC * 64; i += 256) {
            const int t = i & (PCEN_FL_TC - 1), k = i / PCEN_FL_TC;
            if (t < tc) xs[t][k] = (kb + k < BINS) ? mag[(size_t)(kb + k) * NP + col0 + t0 + t] : 0.f;
        }
        __syncthreads();
        if (tid < 64) {
            for (int t = 0; t < tc; ++t) {
                const float v = xs[t][tid];
                M = (t0 + t == 0) ? s * v : (1.f - s) * M + s * v;
                xs[t][tid] = M;
            }
        }
        __syncthreads();
        for (int i = tid; i < PCEN_FL_TC * 64; i += 256) {
            const int t = i & (PCEN_FL_TC - 1), k = i / PCEN_FL_TC;
            if (t < tc && kb + k < BINS) out[(size_t)(kb + k) * NP + col0 + t0 + t] = xs[t][k];
        }
        __syncthreads();
    }
}

// pcen_pow_kernel on [257][NP]: grid (NP / 256, 257); columns n >= N are written as zero
__global__ __launch_bounds__(256) void pcen_pow_fl_kernel(const float* __restrict__ mag, float* __restrict__ out, int N,
                                                          int NP, float eps, float alpha, float delta, float r, float dr) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const size_t i = (size_t)blockIdx.y * NP + n;
    out[i] = (n < N) ? pcen_value(mag[i], out[i], eps, alpha, delta, r, dr) : 0.f;
}

// grid NP / FLG; net_out: [8][257][NP]; frames: (B, T, 512) as mask_istft_frames_kernel writes them
__global__ __launch_bounds__(256) void mask_istft_frames_fl_kernel(const float* __restrict__ net_out,
                                                                   float* __restrict__ frames, const cpx* __restrict__ tw,
                                                                   int T, int N, int NP, float beta) {
    __shared__ cpx sa[NF], sb[NF], stw[NF / 2];
    __shared__ cpx sx[FLG + 2][BINS];          // rows 0 and FLG + 1: the frames n0 - 1 and n0 + FLG (partners across the edges)
    const int n0 = blockIdx.x * FLG;
    fl_stage_twiddles(stw, tw);
    if (n0 >= N) return;
    const size_t plane = (size_t)BINS * NP;
    const int fn = threadIdx.x & (FLG - 1);
    if (n0 + fn < N) {
#pragma unroll 4                               // (registers are free at two workgroups per CU: several bins' loads in flight)
        for (int k = threadIdx.x / FLG; k < BINS; k += 256 / FLG)
            sx[1 + fn][k] = masked_bin(net_out + (size_t)k * NP + n0 + fn, plane, k, true, beta);
    } else {
        for (int k = threadIdx.x / FLG; k < BINS; k += 256 / FLG) sx[1 + fn][k] = masked_bin(nullptr, plane, k, false, beta);
    }
    for (int i = threadIdx.x; i < 2 * BINS; i += 256) {
        const int side = i / BINS, k = i - side * BINS;
        const int n = side ? n0 + FLG : n0 - 1;
        const bool valid = n >= 0 && n < N;
        sx[side ? FLG + 1 : 0][k] = masked_bin(net_out + (size_t)k * NP + (valid ? n : 0), plane, k, valid, beta);
    }
    __syncthreads();
    fl_each_pair(n0, N, T, [](int, int, int) { return make_float2(0.f, 0.f); },      // nothing to stage from global memory
                 [&](int b, int t0, int slot, cpx, cpx) {
        for (int k = threadIdx.x; k < BINS; k += 256) {
            cpx X1 = sx[slot + 2][k];
            if (t0 + 1 >= T) X1 = make_float2(0.f, 0.f);          // (that row is the next utterance's first frame)
            pack_pair(sa, k, sx[slot + 1][k], X1);
        }
        const cpx* z = fft_lds_t<9, true>(sa, sb, stw);
        for (int i = threadIdx.x; i < NF; i += 256) {
            const cpx v = z[i];
            if (slot >= 0) frames[((size_t)b * T + t0) * NF + i] = v.x * (1.f / NF);
            if (t0 + 1 < T && slot + 1 < FLG) frames[((size_t)b * T + t0 + 1) * NF + i] = v.y * (1.f / NF);
        }
        if (z != sb) __syncthreads();          // (folds away: the result lies in sb, and the transform is done with sa)
    });
}

// grid NP / FLG; g_audio (B, L), net_out [8][257][NP] -> g_net [8][257][NP] with zero columns n >= N
__global__ __launch_bounds__(256) void mask_istft_bwd_fl_kernel(const float* __restrict__ g_audio,
                                                                const float* __restrict__ net_out,
                                                                float* __restrict__ g_net, const cpx* __restrict__ tw,
                                                                int T, int L, int N, int NP, float beta) {
    __shared__ cpx sa[NF], sb[NF], stw[NF / 2];
    __shared__ cpx sx[FLG][BINS];
    const int n0 = blockIdx.x * FLG;
    fl_stage_twiddles(stw, tw);
    fl_each_pair(n0, N, T,
                 [&](int b, int t0, int i) { return load_grad_pair(g_audio + (size_t)b * L, t0, T, L, i); },
                 [&](int b, int t0, int slot, cpx v0, cpx v1) {
        sa[threadIdx.x] = v0;
        sa[threadIdx.x + 256] = v1;
        const cpx* Z = fft_lds_t<9, false>(sa, sb, stw);
        for (int k = threadIdx.x; k < BINS; k += 256) {
            cpx G[2];
            split_pair(Z, k, NF, G[0], G[1]);
#pragma unroll
            for (int f = 0; f < 2; ++f)
                if (t0 + f < T && slot + f >= 0 && slot + f < FLG) sx[slot + f][k] = G[f];
        }
        if (Z != sb) __syncthreads();          // (folds away: the result lies in sb, and the transform is done with sa)
    });
    __syncthreads();
    const int fn = threadIdx.x & (FLG - 1);
    const int n = n0 + fn;
    const size_t plane = (size_t)BINS * NP;
    if (n < N) {
#pragma unroll 4                               // (registers are free at two workgroups per CU: several bins' loads in flight)
        for (int k = threadIdx.x / FLG; k < BINS; k += 256 / FLG) {
            const size_t base = (size_t)k * NP + n;
            mask_bwd_bin(net_out + base, g_net + base, plane, sx[fn][k], k, beta);
        }
    } else {
        for (int k = threadIdx.x / FLG; k < BINS; k += 256 / FLG)
#pragma unroll
            for (int c = 0; c < 8; ++c) g_net[(size_t)k * NP + n + c * plane] = 0.f;
    }
}

// ---------------------------------------------------------------- causal audio-in -> audio-out stream (stream.py:83-109)
// One new hop of 128 samples per stream and call.  State per stream: the last 512 input samples (`ring`), the PCEN
// smoother M (dataset.py:56-76: M[t] = (1-s) M[t-1] + s x[t], M[0] = s x[0]) and the overlap-add tail of the output.
// stream_features_kernel: ring <- [ring[128:], chunk] (chunk == NULL: the ring already holds the frame), rect-window
// rFFT-512 of the ring = ONE STFT frame of dataset.py:246-272 (the frame the centred STFT produces two hops later), the same
// arithmetic per bin as stft_features_kernel / pcen_*_kernel, PCEN with the carried state.  Block = two streams (two real
// frames share one complex FFT); feat: (S, C, 257).
__global__ __launch_bounds__(256) void stream_features_kernel(float* __restrict__ ring, const float* __restrict__ chunk,
                                                              float* __restrict__ pcen_M, float* __restrict__ feat,
                                                              const cpx* __restrict__ tw, int S, int C, int first, float eps,
                                                              float s, float alpha, float delta, float r, float dr) {
    __shared__ cpx sa[NF], sb[NF];
    __shared__ int wl[4];
    const int s0 = blockIdx.x * 2;
    const bool two = s0 + 1 < S;
    cpx st[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = threadIdx.x + 256 * h;
        float v[2] = {0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (f == 1 && !two) continue;
            float* rg = ring + (size_t)(s0 + f) * NF;
            if (chunk) v[f] = (i < NF - HOPF) ? rg[i + HOPF] : chunk[(size_t)(s0 + f) * HOPF + (i - (NF - HOPF))];
            else v[f] = rg[i];
        }
        st[h] = make_float2(v[0], v[1]);
    }
    stage_pair(sa, wl, st[0], st[1]);
    __syncthreads();                      // every old ring sample has been read before the shifted ring is written
    if (chunk) {
        for (int i = threadIdx.x; i < NF; i += 256) {
            ring[(size_t)s0 * NF + i] = sa[i].x;
            if (two) ring[(size_t)(s0 + 1) * NF + i] = sa[i].y;
        }
    }
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    const int live = pair_live(wl);
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
        split_pair(Z, k, NF, X[0], X[1]);
        silence_pair(live, X[0], X[1]);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            if (f == 1 && !two) continue;
            float nm, sn, cs;
            const float mag = spectral_features(X[f].x, X[f].y, nm, sn, cs);
            float* o = feat + ((size_t)(s0 + f) * C) * BINS + k;
            o[0] = nm;
            o[(size_t)(C - 2) * BINS] = sn;
            o[(size_t)(C - 1) * BINS] = cs;
            if (C == 4) {
                float* Mp = pcen_M + (size_t)(s0 + f) * BINS + k;
                const float M = first ? s * mag : (1.f - s) * (*Mp) + s * mag;
                *Mp = M;
                o[BINS] = pcen_value(mag, M, eps, alpha, delta, r, dr);
            }
        }
    }
}

// stream_mask_istft_kernel: net output of ONE frame per stream (S, 8, 257) -> phase-aware mask -> irFFT-512 (the arithmetic
// of mask_istft_frames_kernel) -> overlap-add into the stream's tail `ola` (512 partial sums of the padded positions
// [128 t, 128 t + 512), frames added in ascending order like ola_kernel) -> the 128 samples that are final now, divided by
// the number of frames that cover them (`env`: 4 in steady state, fewer at the ends of an utterance) -> tail shifted by a hop.
__global__ __launch_bounds__(256) void stream_mask_istft_kernel(const float* __restrict__ net_out, float* __restrict__ ola,
                                                                float* __restrict__ out, const cpx* __restrict__ tw, int S,
                                                                float beta, float env) {
    __shared__ cpx sa[NF], sb[NF];
    const int s0 = blockIdx.x * 2;
    const bool two = s0 + 1 < S;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            X[f] = make_float2(0.f, 0.f);
            if (f == 0 || two) {
                const MaskVals v = mask_vals(net_out + (size_t)(s0 + f) * 8 * BINS + k, BINS, beta);
                const float M = v.S * v.A;
                X[f] = make_float2(M * v.cm, M * v.sm);
            }
            if (k == 0 || k == NF / 2) X[f].y = 0.f;
        }
        sa[k] = make_float2(X[0].x - X[1].y, X[0].y + X[1].x);
        if (k > 0 && k < NF / 2) sa[NF - k] = make_float2(X[0].x + X[1].y, -X[0].y + X[1].x);
    }
    const cpx* z = fft_lds_t<9, true>(sa, sb, tw);
    cpx* acc = (z == sa) ? sb : sa;       // the other buffer: free after the transform
    for (int i = threadIdx.x; i < NF; i += 256) {
        const cpx v = z[i];
        float a0 = ola[(size_t)s0 * NF + i] + v.x * (1.f / NF);
        float a1 = two ? ola[(size_t)(s0 + 1) * NF + i] + v.y * (1.f / NF) : 0.f;
        acc[i] = make_float2(a0, a1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NF; i += 256) {
        const cpx nx = (i + HOPF < NF) ? acc[i + HOPF] : make_float2(0.f, 0.f);
        ola[(size_t)s0 * NF + i] = nx.x;
        if (two) ola[(size_t)(s0 + 1) * NF + i] = nx.y;
        if (i < HOPF) {
            out[(size_t)s0 * HOPF + i] = acc[i].x / env;
            if (two) out[(size_t)(s0 + 1) * HOPF + i] = acc[i].y / env;
        }
    }
}

// The three per-element expressions every pool path shares (the _rows kernels below and the feed kernels after them): a
// session's samples are the same bits whichever of the two ingests it, so the expressions exist once.
//   pcen_smooth: the PCEN smoother, M[0] = s x[0], M[t] = (1 - s) M[t-1] + s x[t] (below)
//   ola_add:     one frame sample (unnormalised inverse transform) onto the overlap-add tail
//   env_div:     a completed sample over the number of frames that cover it
// The smoother rounds both products and then adds them, the form the _rows kernel has always compiled to (its two products
// share a v_pk_mul_f32).  Contraction is switched off for it: left to the compiler, `(1 - s) M + s x` stays that way in one
// kernel and becomes one fused multiply-add in another -- a last-bit difference between the two ingests of the pool.
__device__ __forceinline__ float pcen_smooth(bool first, float M, float mag, float s) {
#pragma clang fp contract(off)
    const float sx = s * mag;
    return first ? sx : (1.f - s) * M + sx;
}
__device__ __forceinline__ float ola_add(float prev, float z) { return prev + z * (1.f / NF); }
__device__ __forceinline__ float env_div(float v, float env) { return v / env; }

// ---------------------------------------------------------------- stream pool: independent sessions behind a row table
// The lockstep kernels above give every stream the same `first` / `env` and pack streams 2i and 2i+1 into one complex FFT, so a
// stream's last bits depend on its neighbour.  The pool (streaming.StreamPool) runs sessions that start, pause and end on their
// own: a launch handles the ROWS of one pass, row i works on state slot rows[i].slot, and what was a host scalar is per-row
// data.  One real frame per workgroup (imaginary half zero: X[k] = Z[k]; the inverse transforms the Hermitian extension and
// keeps the real part), so nothing a row computes depends on any other row of the launch, bit for bit.  The one pairing is
// inside a session: frames 0 and 1, which a session owes at the same moment, share one transform exactly as the offline
// kernels pair them (TRUNET_ROW_FIRST; frame 1 waits in `stash` (slots, C, 257) for the next pass, TRUNET_ROW_STASHED).
// Frame 0 is symmetric about sample 256, its spectrum real up to (-1)^k with zero crossings between bins: the features of a
// bin next to a crossing are decided by the rounding of the transform, so this frame is computed the way enhance computes it.
// Row record = TRUNET_ROW_INTS int32 (trunet_hip.h):
//   [0] slot  [1] flags  [2] t  [3] a  [4] tail  [5] env  [6] chunk row  [7] out row (-1: none)
// with t the frame index and a the whole hops received (after this row's shift), tail the 0..127 samples after the last whole
// hop of a closing session.  Frame t of the centred STFT is x[reflect(128 t + i - 256, L)], L = 128 a + tail; the ring holds
// x[128 a - 512, 128 a) and the chunk row holds the tail, so every frame of a session's life -- the reflect-built frames 0
// and 1, the steady state (t = a - 2: the ring as it is) and the end frames at any length -- is built here from kept samples.
// Sample positions are taken from an origin that moves with the session (a -> min(a, 4), t by the same amount: a frame is
// computed while t >= a - 2, so nothing left of the origin is ever needed), which keeps 128 t small however old a session is.
// A row whose slot, chunk row, feature row or out row lies outside the given extents is skipped by its whole workgroup
// before it touches memory; sample indices are clamped into the staged 640 samples whatever t, a and tail say.
constexpr int ROW_INTS = TRUNET_ROW_INTS;
constexpr int POOL_XS = NF + HOPF;

// grid (rows); feat (n_frames, C, 257): row i < n_frames writes feat[i], rows from n_frames on only store their hop
__global__ __launch_bounds__(256) void stream_features_rows_kernel(float* __restrict__ ring, const float* __restrict__ chunks,
                                                                   float* __restrict__ pcen_M, float* __restrict__ stash,
                                                                   float* __restrict__ feat,
                                                                   const int* __restrict__ rows, int n_frames, int n_chunks,
                                                                   int slots, const cpx* __restrict__ tw, int C, float eps,
                                                                   float s, float alpha, float delta, float r, float dr) {
    __shared__ cpx sa[NF], sb[NF];
    __shared__ float xs[POOL_XS];
    __shared__ int wl[4];
    const int row = blockIdx.x;
    const int* rec = rows + (size_t)row * ROW_INTS;
    const int slot = rec[0], flags = rec[1], crow = rec[6];
    const int a = min(max(rec[3], 0), 4), t = min(max(rec[2] - (rec[3] - a), 0), 4);
    const int tail = min(max(rec[4], 0), HOPF - 1);
    const bool shift = (flags & TRUNET_ROW_SHIFT) != 0, frame = (flags & TRUNET_ROW_NOFRAME) == 0;
    // all of this is uniform over the workgroup: a bad row leaves without a load or a store
    if (slot < 0 || slot >= slots) return;
    if ((shift || tail > 0) && (crow < 0 || crow >= n_chunks)) return;
    if (frame && row >= n_frames) return;
    float* rg = ring + (size_t)slot * NF;
    for (int i = threadIdx.x; i < POOL_XS; i += 256) {
        float v = 0.f;
        if (i < NF) {
            if (shift) v = (i < NF - HOPF) ? rg[i + HOPF] : chunks[(size_t)crow * HOPF + (i - (NF - HOPF))];
            else v = rg[i];
        } else if (!shift && i - NF < tail) {
            v = chunks[(size_t)crow * HOPF + (i - NF)];
        }
        xs[i] = v;
    }
    __syncthreads();                      // every old ring sample has been read before the shifted ring is written
    if (shift) {
        for (int i = threadIdx.x; i < NF; i += 256) rg[i] = xs[i];
    }
    if (!frame) return;
    float* o = feat + ((size_t)row * C) * BINS;
    float* sh = stash + ((size_t)slot * C) * BINS;
    if (flags & TRUNET_ROW_STASHED) {                     // frame 1: computed with frame 0, one pass earlier
        for (int i = threadIdx.x; i < C * BINS; i += 256) o[i] = sh[i];
        return;
    }
    const bool first = (flags & TRUNET_ROW_FIRST) != 0;   // frame 0, and frame 1 in the imaginary half
    const int L = a * HOPF + tail, base = a * HOPF - NF;
    cpx st[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = threadIdx.x + 256 * h;
        const int j = reflect_idx(t * HOPF + i - NF / 2, L) - base;
        float v1 = 0.f;
        if (first) {
            const int j1 = reflect_idx((t + 1) * HOPF + i - NF / 2, L) - base;
            v1 = xs[min(max(j1, 0), POOL_XS - 1)];
        }
        st[h] = make_float2(xs[min(max(j, 0), POOL_XS - 1)], v1);
    }
    stage_pair(sa, wl, st[0], st[1]);
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    const int live = pair_live(wl);
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X = Z[k], X1 = make_float2(0.f, 0.f);
        if (first) { split_pair(Z, k, NF, X, X1); silence_pair(live, X, X1); }
        float nm, sn, cs;
        const float mag = spectral_features(X.x, X.y, nm, sn, cs);
        o[k] = nm;
        o[(size_t)(C - 2) * BINS + k] = sn;
        o[(size_t)(C - 1) * BINS + k] = cs;
        float M = 0.f;
        if (C == 4) {
            float* Mp = pcen_M + (size_t)slot * BINS + k;
            M = pcen_smooth(first, first ? 0.f : *Mp, mag, s);
            if (!first) *Mp = M;
            o[BINS + k] = pcen_value(mag, M, eps, alpha, delta, r, dr);
        }
        if (first) {
            const float mag1 = spectral_features(X1.x, X1.y, nm, sn, cs);
            sh[k] = nm;
            sh[(size_t)(C - 2) * BINS + k] = sn;
            sh[(size_t)(C - 1) * BINS + k] = cs;
            if (C == 4) {
                M = pcen_smooth(false, M, mag1, s);
                pcen_M[(size_t)slot * BINS + k] = M;
                sh[BINS + k] = pcen_value(mag1, M, eps, alpha, delta, r, dr);
            }
        }
    }
}

// grid (rows); net_out (rows, 8, 257) -> mask -> irFFT-512 -> the slot's overlap-add tail (TRUNET_ROW_FIRST: the tail starts
// from zero, whatever the slot's last session left) -> out[out row] = the hop that is final now / env; tail shifted by a hop.
// TRUNET_ROW_FINISH (the last frame of a session): the two pieces no later frame will touch follow in out rows + 1 and + 2:
// the last whole hop (three frames cover it) and the hop that holds the tail samples (two frames).
__global__ __launch_bounds__(256) void stream_mask_istft_rows_kernel(const float* __restrict__ net_out, float* __restrict__ ola,
                                                                     float* __restrict__ out, const int* __restrict__ rows,
                                                                     int n_out, int slots, const cpx* __restrict__ tw,
                                                                     float beta) {
    __shared__ cpx sa[NF], sb[NF];
    const int row = blockIdx.x;
    const int* rec = rows + (size_t)row * ROW_INTS;
    const int slot = rec[0], flags = rec[1], env = rec[5], orow = rec[7];
    const bool finish = (flags & TRUNET_ROW_FINISH) != 0;
    if (slot < 0 || slot >= slots || env < 1) return;                          // uniform over the workgroup
    if (orow >= 0 ? orow + (finish ? 3 : 1) > n_out : finish) return;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        const MaskVals v = mask_vals(net_out + (size_t)row * 8 * BINS + k, BINS, beta);
        const float M = v.S * v.A;
        cpx X = make_float2(M * v.cm, M * v.sm);
        if (k == 0 || k == NF / 2) X.y = 0.f;            // c2r ignores the imaginary part of DC / Nyquist
        sa[k] = X;
        if (k > 0 && k < NF / 2) sa[NF - k] = make_float2(X.x, -X.y);
    }
    const cpx* z = fft_lds_t<9, true>(sa, sb, tw);
    float* acc = (float*)((z == sa) ? sb : sa);           // the other buffer: free after the transform
    float* ol = ola + (size_t)slot * NF;
    const bool first = (flags & TRUNET_ROW_FIRST) != 0;
    for (int i = threadIdx.x; i < NF; i += 256) acc[i] = ola_add(first ? 0.f : ol[i], z[i].x);
    __syncthreads();
    const float fenv = (float)env;
    for (int i = threadIdx.x; i < NF; i += 256) {
        ol[i] = (i + HOPF < NF) ? acc[i + HOPF] : 0.f;
        if (i < HOPF && orow >= 0) out[(size_t)orow * HOPF + i] = env_div(acc[i], fenv);
    }
    if (finish && threadIdx.x < HOPF) {
        out[(size_t)(orow + 1) * HOPF + threadIdx.x] = env_div(acc[HOPF + threadIdx.x], 3.f);
        out[(size_t)(orow + 2) * HOPF + threadIdx.x] = env_div(acc[2 * HOPF + threadIdx.x], 2.f);
    }
}

// ---------------------------------------------------------------- stream pool: packets of any size (StreamPool.feed)
// A call brings every listed session a packet of any length; the session's new whole hops -- none, one or hundreds -- are all
// computed in that call.  Per slot the pool keeps a FIFO of the 0..127 samples that wait for their hop to fill, and a frame of
// the call is a 512-sample window of the session's LINE
//     line = ring[slot] (512: x[128 a0 - 512, 128 a0))  ++  fifo[slot][0, r0)  ++  samples[poff, poff + n)
// (a0 whole hops and r0 pending samples before the call, n the packet).  Four stages, each one launch whatever the sessions and
// the burst lengths are:
//   stream_feed_features   one workgroup per FRAME: the window from the line, the real-frame transform of
//                          stream_features_rows_kernel (frames 0 and 1 of a session in one transform, as there), the spectral
//                          features; with C = 4 the magnitude is left in the PCEN channel
//   stream_feed_commit     one workgroup per SESSION: the PCEN smoother over the session's new frames in frame order (pcen_smooth
//                          / pcen_value per bin, the magnitudes replaced in place), then the slot's ring and FIFO move on by the
//                          call's whole hops.  A later launch than the frames: they all read the ring this one writes
//   stream_feed_mask_istft one workgroup per frame: mask, Hermitian extension, inverse transform -> frames (n_rows, 512)
//   stream_feed_ola        one workgroup per session: its frames onto the slot's overlap-add tail in ascending frame order
//                          (ola_add), every completed hop over its envelope count (env_div), the tail shifted by a hop each time
// Frame record = TRUNET_FEED_INTS int32; record i describes feature row i = net_out row i = frames row i:
//   [0] slot  [1] flags (TRUNET_ROW_FIRST: frame 0, which also computes the session's frame 1 into row [9];
//   TRUNET_ROW_STASHED: frame 1, nothing to transform)  [2] t (informative)  [3] offset of the window's first sample in the
//   line (FIRST: of x[0])  [4] r0  [5] n  [6] poff  [7] env  [8] hop of `out` the completed hop goes to, -1: none  [9] FIRST: row
//   of frame 1, else -1
// Session record = TRUNET_FEED_INTS int32:
//   [0] slot  [1] flags (unused by the kernels)  [2] seq0  [3] frames  [4] whole hops gained  [5] r0  [6] n  [7] poff  [8] r1
//   [9] position in the call (informative); seq[seq0 .. seq0 + frames) are the session's frame records in frame order.
// A record whose slot, sample range, frame list or out hop lies outside the declared extents is skipped by its whole workgroup
// before any load from or store to the state and data buffers; line indices are clamped into the line.
constexpr int FEED_INTS = TRUNET_FEED_INTS;

struct FeedLine {
    const float* rg;
    const float* ff;
    const float* pk;
    int r0, n;
};

// slot and sample range of a record against the extents (uniform over the workgroup)
__device__ __forceinline__ bool feed_line_ok(int slot, int r0, int n, int poff, int slots, int n_samples) {
    return slot >= 0 && slot < slots && r0 >= 0 && r0 < HOPF && n >= 0 && poff >= 0 && n <= n_samples && poff <= n_samples - n;
}

__device__ __forceinline__ float feed_line_at(const FeedLine& l, int i) {
    i = min(max(i, 0), NF + l.r0 + l.n - 1);
    if (i < NF) return l.rg[i];
    if (i < NF + l.r0) return l.ff[i - NF];
    return l.pk[i - NF - l.r0];
}

// grid (n_rows); feat (n_rows, C, 257)
__global__ __launch_bounds__(256) void stream_feed_features_kernel(const float* __restrict__ ring, const float* __restrict__ fifo,
                                                                   const float* __restrict__ samples, float* __restrict__ feat,
                                                                   const int* __restrict__ rows, int n_rows, int n_samples,
                                                                   int slots, const cpx* __restrict__ tw, int C) {
    __shared__ cpx sa[NF], sb[NF];
    __shared__ int wl[4];
    const int row = blockIdx.x;
    const int* rec = rows + (size_t)row * FEED_INTS;
    const int slot = rec[0], flags = rec[1], voff = rec[3], r0 = rec[4], n = rec[5], poff = rec[6], pair = rec[9];
    if (flags & TRUNET_ROW_STASHED) return;              // frame 1: written by the session's FIRST row
    const bool first = (flags & TRUNET_ROW_FIRST) != 0;
    // all of this is uniform over the workgroup: a bad record leaves without a load or a store
    if (!feed_line_ok(slot, r0, n, poff, slots, n_samples)) return;
    if (voff < 0 || voff > r0 + n - (first ? 3 * HOPF - NF : 0)) return;       // FIRST needs x[0, 384), a frame its 512 samples
    if (first && (pair < 0 || pair >= n_rows || pair == row)) return;
    const FeedLine ln = {ring + (size_t)slot * NF, fifo + (size_t)slot * HOPF, samples + poff, r0, n};
    cpx st[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = threadIdx.x + 256 * h;
        float v0, v1 = 0.f;
        if (first) {
            v0 = feed_line_at(ln, voff + reflect_idx(i - NF / 2, 3 * HOPF));
            v1 = feed_line_at(ln, voff + reflect_idx(HOPF + i - NF / 2, 3 * HOPF));
        } else {
            v0 = feed_line_at(ln, voff + i);
        }
        st[h] = make_float2(v0, v1);
    }
    stage_pair(sa, wl, st[0], st[1]);
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    const int live = pair_live(wl);
    float* o = feat + ((size_t)row * C) * BINS;
    float* o1 = feat + ((size_t)(first ? pair : row) * C) * BINS;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X = Z[k], X1 = make_float2(0.f, 0.f);
        if (first) { split_pair(Z, k, NF, X, X1); silence_pair(live, X, X1); }
        float nm, sn, cs;
        const float mag = spectral_features(X.x, X.y, nm, sn, cs);
        o[k] = nm;
        o[(size_t)(C - 2) * BINS + k] = sn;
        o[(size_t)(C - 1) * BINS + k] = cs;
        if (C == 4) o[BINS + k] = mag;
        if (first) {
            const float mag1 = spectral_features(X1.x, X1.y, nm, sn, cs);
            o1[k] = nm;
            o1[(size_t)(C - 2) * BINS + k] = sn;
            o1[(size_t)(C - 1) * BINS + k] = cs;
            if (C == 4) o1[BINS + k] = mag1;
        }
    }
}

// the frame list of a session against n_rows: true if every entry names a frame record (uniform: ends with a barrier)
__device__ __forceinline__ bool feed_seq_ok(const int* __restrict__ seq, int seq0, int nfr, int n_rows) {
    if (seq0 < 0 || nfr < 0 || nfr > n_rows || seq0 > n_rows - nfr) return false;
    int bad = 0;
    for (int j = threadIdx.x; j < nfr; j += 256) {
        const int r = seq[seq0 + j];
        bad |= (r < 0 || r >= n_rows);
    }
    return __syncthreads_or(bad) == 0;
}

// grid (n_sess)
__global__ __launch_bounds__(256) void stream_feed_commit_kernel(float* __restrict__ ring, float* __restrict__ fifo,
                                                                 const float* __restrict__ samples, float* __restrict__ pcen_M,
                                                                 float* __restrict__ feat, const int* __restrict__ rows,
                                                                 const int* __restrict__ sess, const int* __restrict__ seq,
                                                                 int n_rows, int n_samples, int slots, int C, float eps,
                                                                 float s, float alpha, float delta, float r, float dr) {
    const int* rec = sess + (size_t)blockIdx.x * FEED_INTS;
    const int slot = rec[0], seq0 = rec[2], nfr = rec[3], adv = rec[4], r0 = rec[5], n = rec[6], poff = rec[7], r1 = rec[8];
    if (!feed_line_ok(slot, r0, n, poff, slots, n_samples)) return;
    if (r1 < 0 || r1 >= HOPF || adv < 0 || adv > (r0 + n) / HOPF || r0 + n - adv * HOPF != r1) return;
    if (!feed_seq_ok(seq, seq0, nfr, n_rows)) return;
    if (C == 4 && nfr > 0) {
        for (int k = threadIdx.x; k < BINS; k += 256) {
            float* Mp = pcen_M + (size_t)slot * BINS + k;
            float M = *Mp;
            for (int j = 0; j < nfr; ++j) {
                const int row = seq[seq0 + j];
                const bool first = (rows[(size_t)row * FEED_INTS + 1] & TRUNET_ROW_FIRST) != 0;
                float* o = feat + ((size_t)row * C + 1) * BINS + k;
                const float mag = *o;
                M = pcen_smooth(first, M, mag, s);
                *o = pcen_value(mag, M, eps, alpha, delta, r, dr);
            }
            *Mp = M;
        }
    }
    // ring <- line[128 adv, 128 adv + 512), fifo <- the r1 samples after it: everything is read before anything is written
    const FeedLine ln = {ring + (size_t)slot * NF, fifo + (size_t)slot * HOPF, samples + poff, r0, n};
    const int t = threadIdx.x, base = adv * HOPF;
    const float v0 = feed_line_at(ln, base + t), v1 = feed_line_at(ln, base + 256 + t);
    const float v2 = (t < r1) ? feed_line_at(ln, base + NF + t) : 0.f;
    __syncthreads();
    if (adv > 0) {
        ring[(size_t)slot * NF + t] = v0;
        ring[(size_t)slot * NF + 256 + t] = v1;
    }
    if (t < r1) fifo[(size_t)slot * HOPF + t] = v2;
}

// grid (n_rows); net_out (n_rows, 8, 257) -> frames (n_rows, 512): the real part of the unnormalised inverse transform
__global__ __launch_bounds__(256) void stream_feed_mask_istft_kernel(const float* __restrict__ net_out,
                                                                     float* __restrict__ frames, const cpx* __restrict__ tw,
                                                                     float beta) {
    __shared__ cpx sa[NF], sb[NF];
    const int row = blockIdx.x;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        const MaskVals v = mask_vals(net_out + (size_t)row * 8 * BINS + k, BINS, beta);
        const float M = v.S * v.A;
        cpx X = make_float2(M * v.cm, M * v.sm);
        if (k == 0 || k == NF / 2) X.y = 0.f;            // c2r ignores the imaginary part of DC / Nyquist
        sa[k] = X;
        if (k > 0 && k < NF / 2) sa[NF - k] = make_float2(X.x, -X.y);
    }
    const cpx* z = fft_lds_t<9, true>(sa, sb, tw);
    for (int i = threadIdx.x; i < NF; i += 256) frames[(size_t)row * NF + i] = z[i].x;
}

// grid (sessions that have frames); out (n_out, 128)
__global__ __launch_bounds__(256) void stream_feed_ola_kernel(const float* __restrict__ frames, float* __restrict__ ola,
                                                              float* __restrict__ out, const int* __restrict__ rows,
                                                              const int* __restrict__ sess, const int* __restrict__ seq,
                                                              int n_rows, int n_out, int slots) {
    __shared__ float acc[NF];
    const int* rec = sess + (size_t)blockIdx.x * FEED_INTS;
    const int slot = rec[0], seq0 = rec[2], nfr = rec[3];
    if (slot < 0 || slot >= slots || nfr < 1) return;
    if (!feed_seq_ok(seq, seq0, nfr, n_rows)) return;
    int bad = 0;
    for (int j = threadIdx.x; j < nfr; j += 256) {
        const int* fr = rows + (size_t)seq[seq0 + j] * FEED_INTS;
        bad |= (fr[7] < 1 || fr[8] < -1 || fr[8] >= n_out);
    }
    if (__syncthreads_or(bad)) return;
    const int t = threadIdx.x;
    float* ol = ola + (size_t)slot * NF;
    float t0 = ol[t], t1 = ol[256 + t];
    for (int j = 0; j < nfr; ++j) {
        const int row = seq[seq0 + j];
        const int* fr = rows + (size_t)row * FEED_INTS;
        const bool first = (fr[1] & TRUNET_ROW_FIRST) != 0;
        const int orow = fr[8];
        const float fenv = (float)fr[7];
        acc[t] = ola_add(first ? 0.f : t0, frames[(size_t)row * NF + t]);
        acc[256 + t] = ola_add(first ? 0.f : t1, frames[(size_t)row * NF + 256 + t]);
        __syncthreads();
        if (t < HOPF && orow >= 0) out[(size_t)orow * HOPF + t] = env_div(acc[t], fenv);
        t0 = acc[t + HOPF];
        t1 = (t + HOPF < 256) ? acc[256 + t + HOPF] : 0.f;
        __syncthreads();
    }
    ol[t] = t0;
    ol[256 + t] = t1;
}

// One windowed frame pair z = w x + j w y into LDS, and the n/2 twiddles next to it.  NI = n / 256 is a COMPILE-TIME
// count (2 / 4 / 8 for the three resolutions of config/tiny.json), so that a thread's NI (reflected) samples of both
// signals are requested before the first one is used: as a `for (i = tid; i < n; i += 256)` loop of unknown trip count
// hipcc issued load, wait, LDS store per iteration -- eight L2 round trips in a row at n = 2048, most of the ~12 us a
// block of these kernels took (round 3).  NI = 0: any other n (runtime loops).
// Returns whether this thread staged a tap at which the two windowed signals differ: a frame in which NO thread did holds the
// same data twice, and its two spectra are equal in exact arithmetic -- but not out of the shared transform, whose roundings
// for bin k and bin n - k differ.  The kernels give such a frame |Y| = |X| (stft_same_frame), so that x == y means ym == xm and
// sign(log |X| - log |Y|) == 0 bit for bit, as it does for torch, and not a rounding-sized S1 under a square root and a
// random sign per bin.  Frames that differ anywhere take the arithmetic they always took.
template <int NI, bool YZERO>
__device__ __forceinline__ bool stft_stage_frame(cpx* sa, cpx* stw, const float* __restrict__ xb,
                                                 const float* __restrict__ yb, const float* __restrict__ win,
                                                 const cpx* __restrict__ tw, int f, int hop, int n, int L) {
    if constexpr (NI > 0) {
        float vx[NI], vy[NI], w[NI];
        cpx t[NI / 2 > 0 ? NI / 2 : 1];
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const int i = threadIdx.x + 256 * it;
            const int j = reflect_idx(f * hop + i - n / 2, L);
            vx[it] = xb[j];
            vy[it] = YZERO ? 0.f : yb[j];
            w[it] = win[i];
        }
#pragma unroll
        for (int it = 0; it < NI / 2; ++it) t[it] = tw[threadIdx.x + 256 * it];
        bool diff = false;
#pragma unroll
        for (int it = 0; it < NI; ++it) {
            const cpx z = make_float2(w[it] * vx[it], w[it] * vy[it]);
            diff |= (z.x != z.y);
            sa[threadIdx.x + 256 * it] = z;
        }
#pragma unroll
        for (int it = 0; it < NI / 2; ++it) stw[threadIdx.x + 256 * it] = t[it];
        return diff;
    } else {
        bool diff = false;
        for (int i = threadIdx.x; i < n / 2; i += 256) stw[i] = tw[i];
        for (int i = threadIdx.x; i < n; i += 256) {
            const int j = reflect_idx(f * hop + i - n / 2, L);
            const float w = win[i];
            const cpx z = make_float2(w * xb[j], YZERO ? 0.f : w * yb[j]);
            diff |= (z.x != z.y);
            sa[i] = z;
        }
        return diff;
    }
}

template <bool V> struct SameFrame { static constexpr bool value = V; };
// Every wave leaves "one of my lanes staged a differing tap" in its own flag BEFORE the forward transform; after it (the
// transform ends with a barrier) the four flags answer for the whole block.  No barrier of its own.
__device__ __forceinline__ void stft_note_diff(int* wave_diff, bool diff) {
    const int any = __any(diff ? 1 : 0);
    if ((threadIdx.x & 63) == 0) wave_diff[threadIdx.x >> 6] = any;
}
__device__ __forceinline__ bool stft_same_frame(const int* wave_diff) {
    return (wave_diff[0] | wave_diff[1] | wave_diff[2] | wave_diff[3]) == 0;
}

// ---------------------------------------------------------------- multi-resolution STFT loss
// one block per (frame f, signal b): z = w*x + j w*y -> FFT -> |X|, |Y| -> three sums
template <int NI>
__global__ __launch_bounds__(256) void stft_loss_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ win, const cpx* __restrict__ tw,
                                                            float* __restrict__ partials, int L, int n, int logn, int hop,
                                                            int nframes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    cpx* sa = (cpx*)smraw;
    cpx* sb = sa + n;
    cpx* stw = sb + n;                       // the n/2 twiddles, staged once per block (three table reads per butterfly
                                             // from global memory were most of a stage's latency)
    __shared__ double red[12];
    const int f = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (size_t)b * L;
    const float* yb = y + (size_t)b * L;
    __shared__ int wave_diff[4];
    stft_note_diff(wave_diff, stft_stage_frame<NI, false>(sa, stw, xb, yb, win, tw, f, hop, n, L));
    const cpx* Z = fft_lds_ni<NI, false>(sa, sb, n, logn, stw);
    const bool same = stft_same_frame(wave_diff);
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    // two copies of the loop behind a block-uniform branch: the one every differing frame takes is the code it always was
    auto bins = [&](auto same_frame) {
        for (int k = threadIdx.x; k <= n / 2; k += 256) {
            cpx X, Y;
            split_pair(Z, k, n, X, Y);
            const float xm = sqrtf(fmaxf(X.x * X.x + X.y * X.y, 1e-7f));   // stft_loss.py:30
            const float ym = decltype(same_frame)::value ? xm : sqrtf(fmaxf(Y.x * Y.x + Y.y * Y.y, 1e-7f));
            const float d = ym - xm;
            s1 = fmaf(d, d, s1);
            s2 = fmaf(ym, ym, s2);
            s3 += fabsf(logf(ym) - logf(xm));
        }
    };
    if (same) bins(SameFrame<true>{}); else bins(SameFrame<false>{});
    // three sums of <= 1025 terms: wave shuffles, then the four waves through LDS in fp64 (one barrier instead of the ~30
    // of three tree reductions: they cost more than the FFT itself)
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 3 + 0] = (double)s1; red[wave * 3 + 1] = (double)s2; red[wave * 3 + 2] = (double)s3; }
    __syncthreads();
    if (threadIdx.x < 3) {
        float* pp = partials + ((size_t)b * nframes + f) * 3;
        pp[threadIdx.x] = (float)((red[threadIdx.x] + red[3 + threadIdx.x]) + (red[6 + threadIdx.x] + red[9 + threadIdx.x]));
    }
}

// Forward AND gradient frames of one resolution in one pass (round 4; the train-step path of util.loss_fn).  The loss of one
// resolution is sc = sqrt(S1) / sqrt(S2), mag = S3 / count, so its gradient with respect to a bin's magnitude xm is
//   c_sc (xm - ym) + c_mag sign(log xm - log ym) / xm,   c_sc = g lam_sc / (nres sqrt(S1) sqrt(S2)),  c_mag = g lam_mag / (nres count):
// LINEAR in two coefficients that are only known after the grid-wide sums.  So the block that has the frame's spectrum in
// LDS anyway also forms the two coefficient-free gradient half spectra Gs = (xm - ym) X / xm and Gm = sign(.) X / xm^2,
// sends BOTH through ONE inverse FFT (two real sequences share a complex transform: Z = Herm(Gs) + j Herm(Gm)) and writes the
// two windowed frames; the backward of the step is then a gather of c_sc * fr_sc + c_mag * fr_mag (loss_grad_gather_kernel)
// instead of a second kernel that stages the frame and runs the forward FFT again (stft_bwd_kernel: 0.76 of the 1.37 ms the
// three resolutions took per step).  Same reductions, in the same order, as stft_loss_fwd_kernel: the sums are bit-identical.
template <int NI>
__global__ __launch_bounds__(256) void stft_loss_fwdgrad_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ win, const cpx* __restrict__ tw,
                                                                float* __restrict__ partials, float* __restrict__ fr_sc,
                                                                float* __restrict__ fr_mag, int L, int n, int logn, int hop,
                                                                int nframes, int wl, int left) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    cpx* sa = (cpx*)smraw;
    cpx* sb = sa + n;
    cpx* stw = sb + n;
    __shared__ double red[12];
    const int f = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (size_t)b * L;
    const float* yb = y + (size_t)b * L;
    __shared__ int wave_diff[4];
    stft_note_diff(wave_diff, stft_stage_frame<NI, false>(sa, stw, xb, yb, win, tw, f, hop, n, L));
    cpx* Z = fft_lds_ni<NI, false>(sa, sb, n, logn, stw);
    const bool same = stft_same_frame(wave_diff);
    cpx* other = (Z == sa) ? sb : sa;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    auto bins = [&](auto same_frame) {
        for (int k = threadIdx.x; k <= n / 2; k += 256) {
            cpx X, Y;
            split_pair(Z, k, n, X, Y);
            const float px = X.x * X.x + X.y * X.y;
            const float xm = sqrtf(fmaxf(px, 1e-7f));   // stft_loss.py:30
            const float ym = decltype(same_frame)::value ? xm : sqrtf(fmaxf(Y.x * Y.x + Y.y * Y.y, 1e-7f));
            const float d = ym - xm;
            s1 = fmaf(d, d, s1);
            s2 = fmaf(ym, ym, s2);
            const float dl = logf(xm) - logf(ym);
            s3 += fabsf(-dl);
            cpx Gs = make_float2(0.f, 0.f), Gm = Gs;
            if (px > 1e-7f) {       // clamp(min=1e-7) passes no gradient below the floor
                const float sg = (dl > 0.f) ? 1.f : ((dl < 0.f) ? -1.f : 0.f);
                const float gs = xm - ym, gm = sg / xm;
                Gs = make_float2(gs * X.x / xm, gs * X.y / xm);
                Gm = make_float2(gm * X.x / xm, gm * X.y / xm);
            }
            // a[i] = Re sum_{k <= n/2} Gs[k] w^{ki} as the inverse transform of its Hermitian extension A (A[k] = Gs[k] / 2,
            // A[n-k] = conj(Gs[k]) / 2, A[0] = Re Gs[0], A[n/2] = Re Gs[n/2]); the same for Gm -> B; Z' = A + j B
            if (k == 0 || k == n / 2) {
                other[k] = make_float2(Gs.x, Gm.x);
            } else {
                other[k] = make_float2(0.5f * (Gs.x - Gm.y), 0.5f * (Gs.y + Gm.x));
                other[n - k] = make_float2(0.5f * (Gs.x + Gm.y), 0.5f * (-Gs.y + Gm.x));
            }
        }
    };
    if (same) bins(SameFrame<true>{}); else bins(SameFrame<false>{});
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave * 3 + 0] = (double)s1; red[wave * 3 + 1] = (double)s2; red[wave * 3 + 2] = (double)s3; }
    const cpx* g = fft_lds_ni<NI, true>(other, Z, n, logn, stw);          // (begins and ends with a barrier)
    if (threadIdx.x < 3) {
        float* pp = partials + ((size_t)b * nframes + f) * 3;
        pp[threadIdx.x] = (float)((red[threadIdx.x] + red[3 + threadIdx.x]) + (red[6 + threadIdx.x] + red[9 + threadIdx.x]));
    }
    const size_t fo = ((size_t)b * nframes + f) * wl;
    for (int i = threadIdx.x; i < wl; i += 256) {
        const float w = win[left + i];
        const cpx v = g[left + i];
        fr_sc[fo + i] = w * v.x;
        fr_mag[fo + i] = w * v.y;
    }
}

// The scalar end of the train-step loss (util.py:239-250 + stft_loss.py:151-166) in ONE launch instead of four column
// reductions and ~45 single-element torch kernels: block c reduces one column (the L1 partial sums, then S1, S2, S3 of every
// resolution) in fp64; the block that arrives last does the algebra
//   l1 = sum|d| / (B L);  sc_i = sqrt(S1_i) / sqrt(S2_i);  mag_i = S3_i / count_i;
//   loss = l1 + stft_lambda (lam_sc sum sc_i + lam_mag sum mag_i) / nres
// and writes the coefficients the backward gather needs (for an upstream gradient of 1; the gather multiplies by it).
// vals: [0] loss [1] l1 [2] stft_sc * stft_lambda [3] stft_mag * stft_lambda [4] 1 / (B L) [5 + 2i] c_sc_i [6 + 2i] c_mag_i.
// scratch: 1 + 3 nres doubles + one counter (zero on entry, zero again on exit).
struct LossDesc {
    const float* l1_partials; const float* parts[TRUNET_MAX_RES];
    int n_l1, nres, nrows[TRUNET_MAX_RES]; double l1_count, count[TRUNET_MAX_RES];
    float sc_lambda, mag_lambda, stft_lambda;
};
__global__ __launch_bounds__(1024) void loss_finalize_kernel(const LossDesc d, float* __restrict__ loss_out,
                                                             float* __restrict__ vals, double* __restrict__ scratch) {
    __shared__ double red[16];
    __shared__ int last;
    const int c = blockIdx.x;                  // column: 0 = L1, 1 + 3 i + j = S_{j+1} of resolution i
    const float* src; int rows, stride;
    if (c == 0) { src = d.l1_partials; rows = d.n_l1; stride = 1; }
    else { const int i = (c - 1) / 3; src = d.parts[i] + (c - 1) % 3; rows = d.nrows[i]; stride = 3; }
    double s = 0.0;
    int g = threadIdx.x;
    for (; g + 3 * 1024 < rows; g += 4 * 1024) {
        const float v0 = src[(size_t)g * stride], v1 = src[(size_t)(g + 1024) * stride];
        const float v2 = src[(size_t)(g + 2048) * stride], v3 = src[(size_t)(g + 3072) * stride];
        s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
    }
    for (; g < rows; g += 1024) s += (double)src[(size_t)g * stride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned int* counter = (unsigned int*)(scratch + 1 + 3 * TRUNET_MAX_RES);
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k];
        scratch[c] = t;
        __threadfence();
        last = (atomicAdd(counter, 1u) == gridDim.x - 1);
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    volatile double* sc = scratch;
    const double l1 = fabs(sc[0] / d.l1_count);
    double scs = 0.0, mgs = 0.0;
    for (int i = 0; i < d.nres; ++i) {
        // the float roundings of the unfused path (reduce_cols stores fp32 sums; torch.sqrt / division in fp32)
        const float S1 = (float)sc[1 + 3 * i], S2 = (float)sc[2 + 3 * i], S3 = (float)sc[3 + 3 * i];
        const float r1 = sqrtf(S1), r2 = sqrtf(S2);
        scs += (double)(r1 / r2);
        mgs += (double)(S3 / (float)d.count[i]);
        // S1 == 0 (the prediction equals the target in every bin): sqrt(S1) / sqrt(S2) has gradient 0 there, as torch's norm
        // does; 1 / (r1 r2) would be inf, and inf times the exactly-zero gathered frames NaN in every sample
        vals[5 + 2 * i] = (S1 > 0.f) ? d.stft_lambda * d.sc_lambda / (float)d.nres / (r1 * r2) : 0.f;
        vals[6 + 2 * i] = d.stft_lambda * d.mag_lambda / (float)d.nres / (float)d.count[i];
    }
    const float nres = d.nres > 0 ? (float)d.nres : 1.f;
    const float sc_l = (float)scs * d.sc_lambda / nres * d.stft_lambda, mg_l = (float)mgs * d.mag_lambda / nres * d.stft_lambda;
    const float loss = (float)l1 + (sc_l + mg_l);
    loss_out[0] = loss;
    vals[0] = loss; vals[1] = (float)l1; vals[2] = sc_l; vals[3] = mg_l; vals[4] = (float)(1.0 / d.l1_count);
    for (int i = 0; i < (int)gridDim.x; ++i) scratch[i] = 0.0;       // the contract: the scratch is left all zero
    *counter = 0u;
}

// Gradient of the whole loss with respect to the denoised audio in one gather (no float atomics, deterministic):
//   g_audio[b][j] = g * ( vals[4] sign(audio - clean) + sum_i ( c_sc_i OLA_i(fr_sc_i)[j] + c_mag_i OLA_i(fr_mag_i)[j] ) )
// with OLA_i the overlap-add of resolution i's windowed frames over the reflect-padded signal (ola_gather_kernel's index
// arithmetic), c_* from loss_finalize_kernel and g = the upstream gradient of the loss (device scalar).
struct GatherDesc {
    const float* fr_sc[TRUNET_MAX_RES]; const float* fr_mag[TRUNET_MAX_RES];
    int n[TRUNET_MAX_RES], hop[TRUNET_MAX_RES], wl[TRUNET_MAX_RES], nframes[TRUNET_MAX_RES], nres;
};
__global__ __launch_bounds__(256) void loss_grad_gather_kernel(const GatherDesc d, const float* __restrict__ audio,
                                                               const float* __restrict__ clean,
                                                               const float* __restrict__ vals, const float* __restrict__ gup,
                                                               float* __restrict__ g_audio, int L) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    const float df = audio[(size_t)b * L + j] - clean[(size_t)b * L + j];
    float total = (df > 0.f) ? vals[4] : ((df < 0.f) ? -vals[4] : 0.f);
    for (int r = 0; r < d.nres; ++r) {
        const int n = d.n[r], hop = d.hop[r], wl = d.wl[r], nframes = d.nframes[r], left = (n - wl) / 2;
        const float* fs = d.fr_sc[r] + (size_t)b * nframes * wl;
        const float* fm = d.fr_mag[r] + (size_t)b * nframes * wl;
        float as = 0.f, am = 0.f;
#pragma unroll
        for (int which = 0; which < 3; ++which) {
            int v;
            if (which == 0) v = j;
            else if (which == 1) { if (j == 0) continue; v = -j; }
            else { if (j == L - 1) continue; v = 2 * (L - 1) - j; }
            const int hi = v + n / 2 - left;
            const int lo = v + n / 2 - left - wl + 1;
            if (hi < 0) continue;
            int f0 = lo <= 0 ? 0 : (lo + hop - 1) / hop;
            int f1 = hi / hop;
            if (f1 > nframes - 1) f1 = nframes - 1;
            for (int f = f0; f <= f1; ++f) {
                const size_t o = (size_t)f * wl + (v - f * hop + n / 2 - left);
                as += fs[o];
                am += fm[o];
            }
        }
        total = fmaf(vals[5 + 2 * r], as, fmaf(vals[6 + 2 * r], am, total));
    }
    g_audio[(size_t)b * L + j] = gup[0] * total;
}

// stft() of stft_loss.py:9-30 for two signals at once: magnitudes sqrt(clamp(re^2 + im^2, 1e-7)) as (B, frames, bins)
template <int NI>
__global__ __launch_bounds__(256) void stft_mag_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ win, const cpx* __restrict__ tw,
                                                       float* __restrict__ xmag, float* __restrict__ ymag, int L, int n,
                                                       int logn, int hop, int nframes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    cpx* sa = (cpx*)smraw;
    cpx* sb = sa + n;
    cpx* stw = sb + n;
    const int f = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (size_t)b * L;
    const float* yb = y + (size_t)b * L;
    __shared__ int wave_diff[4];
    stft_note_diff(wave_diff, stft_stage_frame<NI, false>(sa, stw, xb, yb, win, tw, f, hop, n, L));
    const cpx* Z = fft_lds_ni<NI, false>(sa, sb, n, logn, stw);
    const bool same = stft_same_frame(wave_diff);
    const size_t base = ((size_t)b * nframes + f) * (n / 2 + 1);
    auto bins = [&](auto same_frame) {
        for (int k = threadIdx.x; k <= n / 2; k += 256) {
            cpx X, Y;
            split_pair(Z, k, n, X, Y);
            const float xm = sqrtf(fmaxf(X.x * X.x + X.y * X.y, 1e-7f));
            xmag[base + k] = xm;
            if (ymag) ymag[base + k] = decltype(same_frame)::value ? xm : sqrtf(fmaxf(Y.x * Y.x + Y.y * Y.y, 1e-7f));
        }
    };
    if (same) bins(SameFrame<true>{}); else bins(SameFrame<false>{});
}

// out[c] = sum_g partials[g*ncols + c], one block of 1024 threads per column, four loads in flight per thread, fp64
// (with 256 threads and one load in flight the 82k-row tables of the STFT loss took 38 us per launch: pure load latency)
__global__ __launch_bounds__(1024) void reduce_cols_kernel(const float* __restrict__ partials, int nparts, int ncols,
                                                           float* __restrict__ out) {
    __shared__ double red[16];
    const int c = blockIdx.x;
    double s = 0.0;
    int g = threadIdx.x;
    for (; g + 3 * 1024 < nparts; g += 4 * 1024) {
        const float v0 = partials[(size_t)g * ncols + c], v1 = partials[(size_t)(g + 1024) * ncols + c];
        const float v2 = partials[(size_t)(g + 2048) * ncols + c], v3 = partials[(size_t)(g + 3072) * ncols + c];
        s += ((double)v0 + (double)v1) + ((double)v2 + (double)v3);
    }
    for (; g < nparts; g += 1024) s += (double)partials[(size_t)g * ncols + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k];
        out[c] = (float)t;
    }
}

// backward of one resolution.  MAG == false (the losses): per bin
//   g_xm = coef[0] * (xm - ym) + coef[1] * sign(log xm - log ym) / xm
// with coef[0] = g_sc * lam_sc / (nres * sqrt(S1) * sqrt(S2)), coef[1] = g_mag * lam_mag / (nres * count);
// MAG == true (the stand-alone stft() of stft_loss.py:9-30): g_xm = gmag[b][f][k], the cotangent of the magnitudes.
// Either way the frame FFT is recomputed, the gradient half spectrum g_xm * X / xm (zero where clamp(min=1e-7) is
// active) goes through the inverse FFT, and the windowed real part over the window's support is written to `fr`
// (B, frames, wl); ola_gather_kernel sums the frames per sample -- no float atomics.
template <bool MAG, int NI>
__global__ __launch_bounds__(256) void stft_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ win, const cpx* __restrict__ tw,
                                                       const float* __restrict__ coef, const float* __restrict__ gmag,
                                                       int L, int n, int logn, int hop, float* __restrict__ fr, int wl,
                                                       int left) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    cpx* sa = (cpx*)smraw;
    cpx* sb = sa + n;
    cpx* stw = sb + n;
    const int f = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (size_t)b * L;
    const float* yb = MAG ? xb : y + (size_t)b * L;
    __shared__ int wave_diff[4];
    const bool diff = stft_stage_frame<NI, MAG>(sa, stw, xb, yb, win, tw, f, hop, n, L);
    if (!MAG) stft_note_diff(wave_diff, diff);
    cpx* Z = fft_lds_ni<NI, false>(sa, sb, n, logn, stw);
    const bool same = MAG ? false : stft_same_frame(wave_diff);
    cpx* other = (Z == sa) ? sb : sa;
    const float c_sc = MAG ? 0.f : coef[0], c_mag = MAG ? 0.f : coef[1];
    const float* gm_row = MAG ? gmag + ((size_t)b * gridDim.x + f) * (n / 2 + 1) : nullptr;
    // build the half spectrum of gradients in `other` (upper half zero), then inverse FFT, real part
    auto bins = [&](auto same_frame) {
        for (int k = threadIdx.x; k < n; k += 256) {
            cpx G = make_float2(0.f, 0.f);
            if (k <= n / 2) {
                cpx X, Y;
                split_pair(Z, k, n, X, Y);
                const float px = X.x * X.x + X.y * X.y;
                if (px > 1e-7f) {   // clamp(min=1e-7) passes no gradient below the floor
                    const float xm = sqrtf(px);
                    float gm;
                    if (MAG) {
                        gm = gm_row[k];
                    } else {
                        const float ym = decltype(same_frame)::value ? xm : sqrtf(fmaxf(Y.x * Y.x + Y.y * Y.y, 1e-7f));
                        const float dl = logf(xm) - logf(ym);
                        const float sg = (dl > 0.f) ? 1.f : ((dl < 0.f) ? -1.f : 0.f);
                        gm = c_sc * (xm - ym) + c_mag * sg / xm;
                    }
                    G = make_float2(gm * X.x / xm, gm * X.y / xm);
                }
            }
            other[k] = G;
        }
    };
    if (same) bins(SameFrame<true>{}); else bins(SameFrame<false>{});
    const cpx* g = fft_lds_ni<NI, true>(other, Z, n, logn, stw);
    float* fo = fr + ((size_t)b * gridDim.x + f) * wl;
    for (int i = threadIdx.x; i < wl; i += 256) fo[i] = win[left + i] * g[left + i].x;
}

// gx[b][j] = sum over the frames (and, near the ends, the reflected positions) whose window support covers sample j:
// the overlap-add of stft_bwd_kernel's frames as a gather -- no float atomics, deterministic.
__global__ __launch_bounds__(256) void ola_gather_kernel(const float* __restrict__ fr, float* __restrict__ gx, int L, int n,
                                                         int hop, int nframes, int wl, int left) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    const float* fb = fr + (size_t)b * nframes * wl;
    float acc = 0.f;
    // positions v of the reflect-padded signal that map onto sample j: v = j, v = -j (j > 0), v = 2(L-1) - j (j < L-1)
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        int v;
        if (which == 0) v = j;
        else if (which == 1) { if (j == 0) continue; v = -j; }
        else { if (j == L - 1) continue; v = 2 * (L - 1) - j; }
        // frame f covers v when left <= v - f*hop + n/2 < left + wl
        const int hi = v + n / 2 - left;                 // f*hop <= hi
        const int lo = v + n / 2 - left - wl + 1;        // f*hop >= lo
        if (hi < 0) continue;
        int f0 = lo <= 0 ? 0 : (lo + hop - 1) / hop;
        int f1 = hi / hop;
        if (f1 > nframes - 1) f1 = nframes - 1;
        for (int f = f0; f <= f1; ++f) acc += fb[(size_t)f * wl + (v - f * hop + n / 2 - left)];
    }
    gx[(size_t)b * L + j] = acc;
}

__global__ void phm_kernel(const float2* __restrict__ m, const float2* __restrict__ e, float* __restrict__ out,
                           int64_t n, float beta) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 a = m[i], b = e[i];
    const float d = atan2f(a.y, a.x) - atan2f(b.y, b.x);
    out[i] = sqrtf(a.x * a.x + a.y * a.y) / (1.f + expf(-beta * d));
}

// backward of phm_kernel: out = s |m|, s = sigmoid(beta (angle m - angle e)).  Gradients in torch's convention for a real
// loss and complex inputs (d/d re + j d/d im); angle() and abs() pass no gradient at 0, like torch.
__global__ void phm_bwd_kernel(const float2* __restrict__ m, const float2* __restrict__ e, const float* __restrict__ gout,
                               float2* __restrict__ gm, float2* __restrict__ ge, int64_t n, float beta) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float2 a = m[i], b = e[i];
    const float g = gout[i];
    const float d = atan2f(a.y, a.x) - atan2f(b.y, b.x);
    const float sg = 1.f / (1.f + expf(-beta * d));
    const float pa = a.x * a.x + a.y * a.y, pb = b.x * b.x + b.y * b.y;
    const float mag = sqrtf(pa);
    const float gth = g * mag * sg * (1.f - sg) * beta;            // d loss / d (angle m - angle e)
    float2 ra = make_float2(0.f, 0.f), rb = make_float2(0.f, 0.f);
    if (pa > 0.f) {
        ra.x = gth * (-a.y / pa) + g * sg * a.x / mag;
        ra.y = gth * (a.x / pa) + g * sg * a.y / mag;
    }
    if (pb > 0.f) {
        rb.x = -gth * (-b.y / pb);
        rb.y = -gth * (b.x / pb);
    }
    if (gm) gm[i] = ra;
    if (ge) ge[i] = rb;
}

// ---------------------------------------------------------------- ragged (packed) batches: offline enhancement
// B utterances of any lengths L_b packed back to back: sample_off[B+1] over the audio, frame_off[B+1] over the frames
// (T_b = 1 + L_b / 128), pair_off[B+1] over the frame PAIRS (ceil(T_b / 2)).  One workgroup per pair, exactly as the
// dense kernels pair frames 2i and 2i+1 of one utterance (a lone last frame with zeros): a frame's rounding depends on
// its partner through split_pair / the Hermitian packing, so with the same pairs every frame is bit for bit the one the
// dense kernels compute for that utterance alone.  A pair never crosses an utterance boundary.
// The offset tables live on the device and are not trusted: an utterance whose extents do not lie inside the declared
// totals, or are not consistent with each other, is skipped, so no index derived from them leaves the buffers.
struct RaggedUtt { int64_t s0, f0; int L, T; };

__device__ __forceinline__ bool ragged_utt(const int64_t* __restrict__ so, const int64_t* __restrict__ fo, int b,
                                           int64_t nS, int64_t nT, RaggedUtt& u) {
    const int64_t s0 = so[b], s1 = so[b + 1], f0 = fo[b], f1 = fo[b + 1];
    if (s0 < 0 || s1 > nS || s1 - s0 < NF / 2 + 1 || s1 - s0 > 0x7fffffffLL) return false;
    if (f0 < 0 || f1 > nT || f1 - f0 != 1 + (s1 - s0) / HOPF) return false;
    u.s0 = s0; u.f0 = f0; u.L = (int)(s1 - s0); u.T = (int)(f1 - f0);
    return true;
}

// workgroup -> (utterance, first frame t0 of its pair); false: inconsistent tables, nothing to do
__device__ __forceinline__ bool ragged_pair(const int64_t* __restrict__ so, const int64_t* __restrict__ fo,
                                            const int64_t* __restrict__ po, int B, int64_t nS, int64_t nT, int64_t p,
                                            RaggedUtt& u, int& t0) {
    const int b = prefix_find(po, B, p);
    if (!ragged_utt(so, fo, b, nS, nT, u)) return false;
    const int64_t p0 = po[b];
    if (p < p0 || po[b + 1] - p0 != (u.T + 1) / 2 || p - p0 >= (u.T + 1) / 2) return false;
    t0 = (int)(p - p0) * 2;
    return true;
}

// the ragged twin of stft_features_kernel: grid (pairs); feat (sum T, C, 257); mag (optional) (sum T, 257)
__global__ __launch_bounds__(256) void stft_features_ragged_kernel(const float* __restrict__ audio,
                                                                   const int64_t* __restrict__ so,
                                                                   const int64_t* __restrict__ fo,
                                                                   const int64_t* __restrict__ po, float* __restrict__ feat,
                                                                   float* __restrict__ mag_out, const cpx* __restrict__ tw,
                                                                   int B, int64_t nS, int64_t nT, int C) {
    __shared__ cpx sa[NF], sb[NF];
    __shared__ int wl[4];
    RaggedUtt u;
    int t0;
    if (!ragged_pair(so, fo, po, B, nS, nT, blockIdx.x, u, t0)) return;      // uniform over the workgroup
    const int L = u.L, T = u.T;
    const float* x = audio + u.s0;
    stage_audio_pair(sa, wl, x, t0, T, L);
    const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    const int live = pair_live(wl);
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
        split_pair(Z, k, NF, X[0], X[1]);
        silence_pair(live, X[0], X[1]);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int t = t0 + f;
            if (t >= T) continue;
            float nm, sn, cs;
            const float mag = spectral_features(X[f].x, X[f].y, nm, sn, cs);
            float* o = feat + ((size_t)(u.f0 + t) * C) * BINS + k;
            o[0] = nm;
            o[(size_t)(C - 2) * BINS] = sn;
            o[(size_t)(C - 1) * BINS] = cs;
            if (mag_out) mag_out[(size_t)(u.f0 + t) * BINS + k] = mag;
        }
    }
}

// pcen_scan_kernel over each utterance's own frames: grid (B, 5); the smoother restarts at M[0] = s x[0] per utterance
__global__ __launch_bounds__(256) void pcen_scan_ragged_kernel(const float* __restrict__ mag, float* __restrict__ out,
                                                               const int64_t* __restrict__ fo, int64_t nT, int out_stride,
                                                               float s) {
    __shared__ float xs[PCEN_TC][64];
    const int tid = threadIdx.x;
    const int kb = blockIdx.y * 64;
    const int b = blockIdx.x;
    const int64_t f0 = fo[b], f1 = fo[b + 1];
    if (f0 < 0 || f1 > nT || f1 <= f0) return;
    const int64_t T = f1 - f0;
    const float* x = mag + (size_t)f0 * BINS;
    float* o = out + (size_t)f0 * out_stride;
    float M = 0.f;
    for (int64_t t0 = 0; t0 < T; t0 += PCEN_TC) {
        const int tc = (int)min((int64_t)PCEN_TC, T - t0);
        for (int i = tid; i < tc * 64; i += 256) {
            const int t = i >> 6, k = i & 63;
            xs[t][k] = (kb + k < BINS) ? x[(size_t)(t0 + t) * BINS + kb + k] : 0.f;
        }
        __syncthreads();
        if (tid < 64) {
            for (int t = 0; t < tc; ++t) {
                const float v = xs[t][tid];
                M = (t0 + t == 0) ? s * v : (1.f - s) * M + s * v;
                xs[t][tid] = M;
            }
        }
        __syncthreads();
        for (int i = tid; i < tc * 64; i += 256) {
            const int t = i >> 6, k = i & 63;
            if (kb + k < BINS) o[(size_t)(t0 + t) * out_stride + kb + k] = xs[t][k];
        }
        __syncthreads();
    }
}

// pcen_pow_kernel with the rows on the x axis (the y axis of a grid stops at 65535 rows): grid (2 * rows)
__global__ __launch_bounds__(256) void pcen_pow_rows_kernel(const float* __restrict__ mag, float* __restrict__ out,
                                                            int64_t rows, int out_stride, float eps, float alpha,
                                                            float delta, float r, float dr) {
    const int k = (blockIdx.x & 1) * 256 + threadIdx.x;
    const int64_t row = blockIdx.x >> 1;
    if (k >= BINS || row >= rows) return;
    const float v = mag[(size_t)row * BINS + k];
    float* o = out + (size_t)row * out_stride + k;
    const float M = *o;
    *o = pcen_value(v, M, eps, alpha, delta, r, dr);
}

// the ragged twin of mask_istft_frames_kernel: grid (pairs); net_out (sum T, 8, 257) -> frames (sum T, 512)
__global__ __launch_bounds__(256) void mask_istft_frames_ragged_kernel(const float* __restrict__ net_out,
                                                                       float* __restrict__ frames,
                                                                       const int64_t* __restrict__ so,
                                                                       const int64_t* __restrict__ fo,
                                                                       const int64_t* __restrict__ po,
                                                                       const cpx* __restrict__ tw, int B, int64_t nS,
                                                                       int64_t nT, float beta) {
    __shared__ cpx sa[NF], sb[NF];
    RaggedUtt u;
    int t0;
    if (!ragged_pair(so, fo, po, B, nS, nT, blockIdx.x, u, t0)) return;
    const int T = u.T;
    for (int k = threadIdx.x; k < BINS; k += 256) {
        cpx X[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            X[f] = make_float2(0.f, 0.f);
            const int t = t0 + f;
            if (t < T) {
                const MaskVals v = mask_vals(net_out + (size_t)(u.f0 + t) * 8 * BINS + k, BINS, beta);
                const float M = v.S * v.A;
                X[f] = make_float2(M * v.cm, M * v.sm);
            }
            if (k == 0 || k == NF / 2) X[f].y = 0.f;
        }
        sa[k] = make_float2(X[0].x - X[1].y, X[0].y + X[1].x);
        if (k > 0 && k < NF / 2) sa[NF - k] = make_float2(X[0].x + X[1].y, -X[0].y + X[1].x);
    }
    const cpx* z = fft_lds_t<9, true>(sa, sb, tw);
    for (int i = threadIdx.x; i < NF; i += 256) {
        const cpx v = z[i];
        frames[((size_t)u.f0 + t0) * NF + i] = v.x * (1.f / NF);
        if (t0 + 1 < T) frames[((size_t)u.f0 + t0 + 1) * NF + i] = v.y * (1.f / NF);
    }
}

// ola_kernel per packed sample, without the L1 sums, for all L_b samples of each utterance: samples past (T_b - 1) * 128
// take the same envelope formula (the frames that cover them), which is torch.istft(..., length = L_b)
__global__ __launch_bounds__(256) void ola_ragged_kernel(const float* __restrict__ frames, float* __restrict__ audio,
                                                         const int64_t* __restrict__ so, const int64_t* __restrict__ fo,
                                                         int B, int64_t nS, int64_t nT) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nS) return;
    RaggedUtt u;
    const int b = prefix_find(so, B, g);
    if (!ragged_utt(so, fo, b, nS, nT, u) || g < u.s0) return;
    const int j = (int)(g - u.s0);
    if (j >= u.L) return;
    const int T = u.T;
    const float* fr = frames + (size_t)u.f0 * NF;
    const int p = j + NF / 2;
    int hi = p / HOPF; if (hi > T - 1) hi = T - 1;
    int lo = (p - NF + HOPF) / HOPF; if (p - NF + 1 <= 0) lo = 0;
    float s = 0.f;
    for (int t = lo; t <= hi; ++t) s += fr[(size_t)t * NF + (p - t * HOPF)];
    s /= (float)(hi - lo + 1);
    audio[g] = s;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_stft_features(const float* audio, float* feat, float* mag, const float* tw512, int B, int L, int T,
                                    int C, void* stream) {
    if (!audio || !feat || !tw512 || B <= 0 || L < NF / 2 + 1 || T != 1 + L / HOPF || (C != 3 && C != 4)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stft_features_kernel, dim3((T + 1) / 2, B), dim3(256), 0, ST, audio, feat, mag, (const cpx*)tw512, L, T, C);
    return trunet_launch_status();
}

extern "C" int trunet_pcen(const float* mag, float* out, int B, int T, int out_stride, float eps, float s, float alpha,
                           float delta, float r, void* stream) {
    if (!mag || !out || B <= 0 || T <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(pcen_scan_kernel, dim3((BINS + 63) / 64, B), dim3(256), 0, ST, mag, out, T, out_stride, s);
    hipLaunchKernelGGL(pcen_pow_kernel, dim3((BINS + 255) / 256, B * T), dim3(256), 0, ST, mag, out, B * T, out_stride, eps,
                       alpha, delta, r, powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_mask_istft_fwd(const float* net_out, float* frames, float* audio, const float* clean,
                                     float* l1_partials, const float* tw512, int B, int T, int L, float beta, void* stream) {
    if (!net_out || !frames || !audio || !tw512 || B <= 0 || T < 2 || L != (T - 1) * HOPF) return TRUNET_EINVAL;
    hipLaunchKernelGGL(mask_istft_frames_kernel, dim3((T + 1) / 2, B), dim3(256), 0, ST, net_out, frames, (const cpx*)tw512, T, beta);
    hipLaunchKernelGGL(ola_kernel, dim3((L + 255) / 256, B), dim3(256), 0, ST, frames, audio, clean, l1_partials, T, L);
    return trunet_launch_status();
}

extern "C" int trunet_mask_istft_l1_nparts(int B, int L) { return B * ((L + 255) / 256); }

extern "C" int trunet_mask_istft_bwd(const float* g_audio, const float* net_out, float* g_net, const float* tw512, int B,
                                     int T, int L, float beta, void* stream) {
    if (!g_audio || !net_out || !g_net || !tw512 || B <= 0 || T < 2 || L != (T - 1) * HOPF) return TRUNET_EINVAL;
    hipLaunchKernelGGL(mask_istft_bwd_kernel, dim3((T + 1) / 2, B), dim3(256), 0, ST, g_audio, net_out, g_net, (const cpx*)tw512, T, L, beta);
    return trunet_launch_status();
}

// ---- frames-last boundary: x / net_out / g_net are [C][257][NP], N = B T frames, NP a multiple of 256 (the layer kernels' tile)
static bool fl_shape_ok(int B, int T, int NP) {
    return B > 0 && T > 0 && NP > 0 && NP % 256 == 0 && (int64_t)B * T <= NP;
}

extern "C" int trunet_stft_features_fl(const float* audio, float* x, float* mag, const float* tw512, int B, int L, int T,
                                       int C, int NP, void* stream) {
    if (!audio || !x || !tw512 || B <= 0 || L < NF / 2 + 1 || T != 1 + L / HOPF || (C != 3 && C != 4)) return TRUNET_EINVAL;
    if (!fl_shape_ok(B, T, NP)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stft_features_fl_kernel, dim3(NP / FLG), dim3(256), 0, ST, audio, x, mag, (const cpx*)tw512, L, T, C,
                       B * T, NP);
    return trunet_launch_status();
}

extern "C" int trunet_pcen_fl(const float* mag, float* out, int B, int T, int NP, float eps, float s, float alpha,
                              float delta, float r, void* stream) {
    if (!mag || !out || B <= 0 || T <= 0) return TRUNET_EINVAL;
    if (!fl_shape_ok(B, T, NP)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(pcen_scan_fl_kernel, dim3((BINS + 63) / 64, B), dim3(256), 0, ST, mag, out, T, NP, s);
    hipLaunchKernelGGL(pcen_pow_fl_kernel, dim3(NP / 256, BINS), dim3(256), 0, ST, mag, out, B * T, NP, eps, alpha, delta, r,
                       powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_mask_istft_fwd_fl(const float* net_out, float* frames, float* audio, const float* clean,
                                        float* l1_partials, const float* tw512, int B, int T, int L, int NP, float beta,
                                        void* stream) {
    if (!net_out || !frames || !audio || !tw512 || B <= 0 || T < 2 || L != (T - 1) * HOPF) return TRUNET_EINVAL;
    if (!fl_shape_ok(B, T, NP)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(mask_istft_frames_fl_kernel, dim3(NP / FLG), dim3(256), 0, ST, net_out, frames, (const cpx*)tw512, T,
                       B * T, NP, beta);
    hipLaunchKernelGGL(ola_kernel, dim3((L + 255) / 256, B), dim3(256), 0, ST, frames, audio, clean, l1_partials, T, L);
    return trunet_launch_status();
}

extern "C" int trunet_mask_istft_bwd_fl(const float* g_audio, const float* net_out, float* g_net, const float* tw512, int B,
                                        int T, int L, int NP, float beta, void* stream) {
    if (!g_audio || !net_out || !g_net || !tw512 || B <= 0 || T < 2 || L != (T - 1) * HOPF) return TRUNET_EINVAL;
    if (!fl_shape_ok(B, T, NP)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(mask_istft_bwd_fl_kernel, dim3(NP / FLG), dim3(256), 0, ST, g_audio, net_out, g_net, (const cpx*)tw512,
                       T, L, B * T, NP, beta);
    return trunet_launch_status();
}

extern "C" int trunet_l1_grad(const float* den, const float* clean, const float* scale, float* g, int64_t n, void* stream) {
    if (!den || !clean || !scale || !g || n <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(l1_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, den, clean, scale, g, n);
    return trunet_launch_status();
}

extern "C" int trunet_reduce_cols(const float* partials, int nparts, int ncols, float* out, void* stream) {
    if (!partials || !out || nparts <= 0 || ncols <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(reduce_cols_kernel, dim3(ncols), dim3(1024), 0, ST, partials, nparts, ncols, out);
    return trunet_launch_status();
}

// The STFT sizes the loss kernels take: powers of two from 8 to STFT_MAX_N.  (2 n + n / 2) complex values of dynamic LDS is
// 40 KB at n = 2048, inside the 64 KB a kernel gets without raising its limit; n = 4096 would need 80 KB, which no launch
// here asks for, so the host refuses it instead of accepting a size whose launch fails.
constexpr int STFT_MAX_N = 2048;
// log2 n for a power of two in [1, STFT_MAX_N], -1 for anything else (any int: nothing is shifted past the maximum)
static int ilog2(int n) {
    if (n < 1 || n > STFT_MAX_N) return -1;
    int l = 0;
    while ((1 << l) < n) ++l;
    return ((1 << l) == n) ? l : -1;
}

extern "C" int trunet_stft_loss_fwd(const float* x, const float* y, const float* win, const float* tw, float* partials,
                                    int B, int L, int n, int hop, void* stream) {
    const int logn = ilog2(n);
    if (!x || !y || !win || !tw || !partials || B <= 0 || logn < 3 || hop <= 0 || L <= n / 2) return TRUNET_EINVAL;
    const int nframes = 1 + L / hop;
#define FWD_(NI_) hipLaunchKernelGGL(stft_loss_fwd_kernel<NI_>, dim3(nframes, B), dim3(256), (2 * n + n / 2) * sizeof(cpx), ST, x, y, \
                                    win, (const cpx*)tw, partials, L, n, logn, hop, nframes)
    if (n == 512) FWD_(2); else if (n == 1024) FWD_(4); else if (n == 2048) FWD_(8); else FWD_(0);
#undef FWD_
    return trunet_launch_status();
}

extern "C" int trunet_stft_mag(const float* x, const float* y, const float* win, const float* tw, float* xmag, float* ymag,
                               int B, int L, int n, int hop, void* stream) {
    const int logn = ilog2(n);
    if (!x || !win || !tw || !xmag || B <= 0 || logn < 3 || hop <= 0 || L <= n / 2) return TRUNET_EINVAL;
    const int nframes = 1 + L / hop;
#define MAG_(NI_) hipLaunchKernelGGL(stft_mag_kernel<NI_>, dim3(nframes, B), dim3(256), (2 * n + n / 2) * sizeof(cpx), ST, x, y ? y : x, \
                                    win, (const cpx*)tw, xmag, y ? ymag : nullptr, L, n, logn, hop, nframes)
    if (n == 512) MAG_(2); else if (n == 1024) MAG_(4); else if (n == 2048) MAG_(8); else MAG_(0);
#undef MAG_
    return trunet_launch_status();
}

extern "C" int trunet_stft_loss_bwd_gather(const float* x, const float* y, const float* win, const float* tw,
                                           const float* coef, float* frames, float* gx, int B, int L, int n, int hop,
                                           int win_length, void* stream) {
    const int logn = ilog2(n);
    if (!x || !y || !win || !tw || !coef || !frames || !gx || B <= 0 || logn < 3 || hop <= 0 || L <= n / 2 ||
        win_length <= 0 || win_length > n)
        return TRUNET_EINVAL;
    const int nframes = 1 + L / hop;
    const int left = (n - win_length) / 2;
#define BWD_(NI_) hipLaunchKernelGGL((stft_bwd_kernel<false, NI_>), dim3(nframes, B), dim3(256), (2 * n + n / 2) * sizeof(cpx), ST, x, y, \
                                    win, (const cpx*)tw, coef, (const float*)nullptr, L, n, logn, hop, frames, win_length, left)
    if (n == 512) BWD_(2); else if (n == 1024) BWD_(4); else if (n == 2048) BWD_(8); else BWD_(0);
#undef BWD_
    hipLaunchKernelGGL(ola_gather_kernel, dim3((L + 255) / 256, B), dim3(256), 0, ST, frames, gx, L, n, hop, nframes,
                       win_length, left);
    return trunet_launch_status();
}

extern "C" int trunet_stream_features(float* ring, const float* chunk, float* pcen_M, float* feat, const float* tw512, int S,
                                      int C, int first, float eps, float s, float alpha, float delta, float r, void* stream) {
    if (!ring || !feat || !tw512 || S <= 0 || (C != 3 && C != 4) || (C == 4 && !pcen_M)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_features_kernel, dim3((S + 1) / 2), dim3(256), 0, ST, ring, chunk, pcen_M, feat, (const cpx*)tw512,
                       S, C, first, eps, s, alpha, delta, r, powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_stream_mask_istft(const float* net_out, float* ola, float* out, const float* tw512, int S, float beta,
                                        float env, void* stream) {
    if (!net_out || !ola || !out || !tw512 || S <= 0 || !(env >= 1.f)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_mask_istft_kernel, dim3((S + 1) / 2), dim3(256), 0, ST, net_out, ola, out, (const cpx*)tw512, S,
                       beta, env);
    return trunet_launch_status();
}

extern "C" int trunet_stream_features_rows(float* ring, const float* chunks, float* pcen_M, float* stash, float* feat,
                                           const int32_t* rows,
                                           int n_rows, int n_frames, int n_chunks, int slots, const float* tw512, int C,
                                           float eps, float s, float alpha, float delta, float r, void* stream) {
    if (!ring || !stash || !rows || !tw512 || n_rows <= 0 || n_frames < 0 || n_frames > n_rows || n_chunks < 0 || slots <= 0 ||
        (n_frames > 0 && !feat) || (n_chunks > 0 && !chunks) || (C != 3 && C != 4) || (C == 4 && !pcen_M))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_features_rows_kernel, dim3(n_rows), dim3(256), 0, ST, ring, chunks, pcen_M, stash, feat, rows,
                       n_frames,
                       n_chunks, slots, (const cpx*)tw512, C, eps, s, alpha, delta, r, powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_stream_mask_istft_rows(const float* net_out, float* ola, float* out, const int32_t* rows, int n_rows,
                                             int n_out, int slots, const float* tw512, float beta, void* stream) {
    if (!net_out || !ola || !out || !rows || !tw512 || n_rows <= 0 || n_out <= 0 || slots <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_mask_istft_rows_kernel, dim3(n_rows), dim3(256), 0, ST, net_out, ola, out, rows, n_out, slots,
                       (const cpx*)tw512, beta);
    return trunet_launch_status();
}

extern "C" int trunet_stream_feed_features(const float* ring, const float* fifo, const float* samples, float* feat,
                                           const int32_t* rows, int n_rows, int n_samples, int slots, const float* tw512, int C,
                                           void* stream) {
    if (!ring || !fifo || !feat || !rows || !tw512 || n_rows <= 0 || n_samples < 0 || n_samples > TRUNET_FEED_MAX_SAMPLES ||
        (n_samples > 0 && !samples) || slots <= 0 || (C != 3 && C != 4))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_feed_features_kernel, dim3(n_rows), dim3(256), 0, ST, ring, fifo, samples, feat, rows, n_rows,
                       n_samples, slots, (const cpx*)tw512, C);
    return trunet_launch_status();
}

extern "C" int trunet_stream_feed_commit(float* ring, float* fifo, const float* samples, float* pcen_M, float* feat,
                                         const int32_t* rows, const int32_t* sess, const int32_t* seq, int n_sess, int n_rows,
                                         int n_samples, int slots, int C, float eps, float s, float alpha, float delta, float r,
                                         void* stream) {
    if (!ring || !fifo || !sess || n_sess <= 0 || n_rows < 0 || n_samples < 0 || n_samples > TRUNET_FEED_MAX_SAMPLES ||
        (n_samples > 0 && !samples) || slots <= 0 || (n_rows > 0 && (!feat || !rows || !seq)) || (C != 3 && C != 4) || (C == 4 && !pcen_M))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_feed_commit_kernel, dim3(n_sess), dim3(256), 0, ST, ring, fifo, samples, pcen_M, feat, rows, sess,
                       seq, n_rows, n_samples, slots, C, eps, s, alpha, delta, r, powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_stream_feed_mask_istft(const float* net_out, float* frames, int n_rows, const float* tw512, float beta,
                                             void* stream) {
    if (!net_out || !frames || !tw512 || n_rows <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_feed_mask_istft_kernel, dim3(n_rows), dim3(256), 0, ST, net_out, frames, (const cpx*)tw512, beta);
    return trunet_launch_status();
}

extern "C" int trunet_stream_feed_ola(const float* frames, float* ola, float* out, const int32_t* rows, const int32_t* sess,
                                      const int32_t* seq, int n_sess, int n_rows, int n_out, int slots, void* stream) {
    if (!frames || !ola || !rows || !sess || !seq || n_sess <= 0 || n_rows <= 0 || n_sess > n_rows || n_out < 0 ||
        (n_out > 0 && !out) || slots <= 0)
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_feed_ola_kernel, dim3(n_sess), dim3(256), 0, ST, frames, ola, out, rows, sess, seq, n_rows, n_out,
                       slots);
    return trunet_launch_status();
}

extern "C" int trunet_stft_loss_fwdgrad(const float* x, const float* y, const float* win, const float* tw, float* partials,
                                        float* fr_sc, float* fr_mag, int B, int L, int n, int hop, int win_length, void* stream) {
    const int logn = ilog2(n);
    if (!x || !y || !win || !tw || !partials || !fr_sc || !fr_mag || B <= 0 || logn < 3 || hop <= 0 || L <= n / 2 ||
        win_length <= 0 || win_length > n)
        return TRUNET_EINVAL;
    const int nframes = 1 + L / hop;
    const int left = (n - win_length) / 2;
#define FG_(NI_) hipLaunchKernelGGL(stft_loss_fwdgrad_kernel<NI_>, dim3(nframes, B), dim3(256), (2 * n + n / 2) * sizeof(cpx), ST, x, y, \
                                   win, (const cpx*)tw, partials, fr_sc, fr_mag, L, n, logn, hop, nframes, win_length, left)
    if (n == 512) FG_(2); else if (n == 1024) FG_(4); else if (n == 2048) FG_(8); else FG_(0);
#undef FG_
    return trunet_launch_status();
}

extern "C" size_t trunet_loss_scratch_bytes(void) { return (1 + 3 * TRUNET_MAX_RES + 1) * sizeof(double); }

extern "C" int trunet_loss_finalize(const trunet_loss_args* a, float* loss_out, float* vals, void* scratch, void* stream) {
    if (!a || !loss_out || !vals || !scratch || !a->l1_partials || a->n_l1 <= 0 || !(a->l1_count > 0) || a->nres < 0 ||
        a->nres > TRUNET_MAX_RES)
        return TRUNET_EINVAL;
    LossDesc d;
    d.l1_partials = a->l1_partials; d.n_l1 = a->n_l1; d.nres = a->nres; d.l1_count = a->l1_count;
    d.sc_lambda = a->sc_lambda; d.mag_lambda = a->mag_lambda; d.stft_lambda = a->stft_lambda;
    for (int i = 0; i < a->nres; ++i) {
        if (!a->parts[i] || a->nrows[i] <= 0 || !(a->count[i] > 0)) return TRUNET_EINVAL;
        d.parts[i] = a->parts[i]; d.nrows[i] = a->nrows[i]; d.count[i] = a->count[i];
    }
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1 + 3 * a->nres), dim3(1024), 0, ST, d, loss_out, vals, (double*)scratch);
    return trunet_launch_status();
}

extern "C" int trunet_loss_grad_gather(const trunet_loss_gather_args* a, const float* audio, const float* clean,
                                       const float* vals, const float* g_loss, float* g_audio, int B, int L, void* stream) {
    if (!a || !audio || !clean || !vals || !g_loss || !g_audio || B <= 0 || L <= 0 || a->nres < 0 || a->nres > TRUNET_MAX_RES)
        return TRUNET_EINVAL;
    GatherDesc d;
    d.nres = a->nres;
    for (int i = 0; i < a->nres; ++i) {
        if (!a->fr_sc[i] || !a->fr_mag[i] || ilog2(a->n[i]) < 3 || a->hop[i] <= 0 || a->win_length[i] <= 0 ||
            a->win_length[i] > a->n[i] || L <= a->n[i] / 2)
            return TRUNET_EINVAL;
        d.fr_sc[i] = a->fr_sc[i]; d.fr_mag[i] = a->fr_mag[i]; d.n[i] = a->n[i]; d.hop[i] = a->hop[i];
        d.wl[i] = a->win_length[i]; d.nframes[i] = 1 + L / a->hop[i];
    }
    hipLaunchKernelGGL(loss_grad_gather_kernel, dim3((L + 255) / 256, B), dim3(256), 0, ST, d, audio, clean, vals, g_loss,
                       g_audio, L);
    return trunet_launch_status();
}

extern "C" int trunet_stft_mag_bwd(const float* x, const float* win, const float* tw, const float* gmag, float* frames,
                                   float* gx, int B, int L, int n, int hop, int win_length, void* stream) {
    const int logn = ilog2(n);
    if (!x || !win || !tw || !gmag || !frames || !gx || B <= 0 || logn < 3 || hop <= 0 || L <= n / 2 ||
        win_length <= 0 || win_length > n)
        return TRUNET_EINVAL;
    const int nframes = 1 + L / hop;
    const int left = (n - win_length) / 2;
#define BWD_(NI_) hipLaunchKernelGGL((stft_bwd_kernel<true, NI_>), dim3(nframes, B), dim3(256), (2 * n + n / 2) * sizeof(cpx), ST, x, x, \
                                    win, (const cpx*)tw, (const float*)nullptr, gmag, L, n, logn, hop, frames, win_length, left)
    if (n == 512) BWD_(2); else if (n == 1024) BWD_(4); else if (n == 2048) BWD_(8); else BWD_(0);
#undef BWD_
    hipLaunchKernelGGL(ola_gather_kernel, dim3((L + 255) / 256, B), dim3(256), 0, ST, frames, gx, L, n, hop, nframes,
                       win_length, left);
    return trunet_launch_status();
}

extern "C" int trunet_phm_bwd(const float* mix_ri, const float* est_ri, const float* g_out, float* g_mix_ri, float* g_est_ri,
                              int64_t n, float beta, void* stream) {
    if (!mix_ri || !est_ri || !g_out || (!g_mix_ri && !g_est_ri) || n <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(phm_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float2*)mix_ri,
                       (const float2*)est_ri, g_out, (float2*)g_mix_ri, (float2*)g_est_ri, n, beta);
    return trunet_launch_status();
}

extern "C" int trunet_phm_fwd(const float* mix_ri, const float* est_ri, float* out, int64_t n, float beta, void* stream) {
    if (!mix_ri || !est_ri || !out || n <= 0) return TRUNET_EINVAL;
    hipLaunchKernelGGL(phm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, (const float2*)mix_ri,
                       (const float2*)est_ri, out, n, beta);
    return trunet_launch_status();
}

// ---------------------------------------------------------------- ragged (packed) batches
// What the host can see is checked here; the offset tables themselves are checked per utterance on the device.
// sum T_b = B + sum L_b / 128 with L_b >= 257 (so T_b >= 3); sum ceil(T_b / 2) lies in [sum T / 2, (sum T + B) / 2].
static bool ragged_totals_ok(int B, int64_t nS, int64_t nT, int64_t nP) {
    return B > 0 && nS >= (int64_t)B * (NF / 2 + 1) && nS <= (int64_t)0x7fffffff * 256 && nT >= 3LL * B &&
           nT <= nS / HOPF + B && 2 * nP >= nT && 2 * nP <= nT + B && nP <= 0x7fffffff;
}

extern "C" int trunet_stft_features_ragged(const float* audio, const int64_t* sample_off, const int64_t* frame_off,
                                           const int64_t* pair_off, float* feat, float* mag, const float* tw512, int B,
                                           int64_t total_samples, int64_t total_frames, int64_t total_pairs, int C,
                                           void* stream) {
    if (!audio || !sample_off || !frame_off || !pair_off || !feat || !tw512 || (C != 3 && C != 4) ||
        !ragged_totals_ok(B, total_samples, total_frames, total_pairs))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stft_features_ragged_kernel, dim3((unsigned)total_pairs), dim3(256), 0, ST, audio, sample_off,
                       frame_off, pair_off, feat, mag, (const cpx*)tw512, B, total_samples, total_frames, C);
    return trunet_launch_status();
}

extern "C" int trunet_pcen_ragged(const float* mag, float* out, const int64_t* frame_off, int B, int64_t total_frames,
                                  int out_stride, float eps, float s, float alpha, float delta, float r, void* stream) {
    if (!mag || !out || !frame_off || B <= 0 || total_frames < B || total_frames > 0x3fffffff || out_stride < BINS)
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(pcen_scan_ragged_kernel, dim3(B, (BINS + 63) / 64), dim3(256), 0, ST, mag, out, frame_off,
                       total_frames, out_stride, s);
    hipLaunchKernelGGL(pcen_pow_rows_kernel, dim3((unsigned)(2 * total_frames)), dim3(256), 0, ST, mag, out, total_frames,
                       out_stride, eps, alpha, delta, r, powf(delta, r));
    return trunet_launch_status();
}

extern "C" int trunet_mask_istft_ragged(const float* net_out, float* frames, float* audio, const int64_t* sample_off,
                                        const int64_t* frame_off, const int64_t* pair_off, const float* tw512, int B,
                                        int64_t total_samples, int64_t total_frames, int64_t total_pairs, float beta,
                                        void* stream) {
    if (!net_out || !frames || !audio || !sample_off || !frame_off || !pair_off || !tw512 ||
        !ragged_totals_ok(B, total_samples, total_frames, total_pairs))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(mask_istft_frames_ragged_kernel, dim3((unsigned)total_pairs), dim3(256), 0, ST, net_out, frames,
                       sample_off, frame_off, pair_off, (const cpx*)tw512, B, total_samples, total_frames, beta);
    hipLaunchKernelGGL(ola_ragged_kernel, dim3((unsigned)((total_samples + 255) / 256)), dim3(256), 0, ST, frames, audio,
                       sample_off, frame_off, B, total_samples, total_frames);
    return trunet_launch_status();
}
