// Reverberant training data on the GPU: every row of a batch is convolved with its own room impulse response (RIR), an
// optional early-reflections target is produced beside it, the augmented noise is mixed in at a requested SNR and the pair
// is guarded against clipping (float64 statement: tests/reverb_ref.py):
//   wet[n]  = sum_{k < K_b, k <= n} h[k] x[n-k]           (causal, truncated to L; K_b == 0: wet = x bit for bit)
//   tgt     = x (E == 0 or K_b == 0)   else   sum_{k < min(E, K_b)} h[k] x[n-k]
//   g       = sqrt(Ps / (Pv 10^(snr/10))), Ps = mean(wet^2), Pv = mean(v^2)    (1 without snr, or when Ps or Pv < 1e-20)
//   noisy   = wet + g v;   m = max|noisy| > peak > 0  =>  noisy, tgt *= peak / m
//
// The convolution is a uniformly partitioned overlap-save convolution, partition P = 1024 taps, transform N = 2048, on the
// in-LDS Stockham FFT of fft_common.hpp.  Real sequences ride two per complex transform (split_pair):
//   reverb_spectra_kernel   signal windows j, j+1 -> X[b][j], X[b][j+1];  RIR partitions p, p+1 -> H[b][p], H[b][p+1];
//                           the early target's cut partition -> H[b][nP]
//   reverb_conv_kernel      one workgroup per (row, output block j): W = sum_p X[j-p] H[p] over the row's OWN partition count
//                           (ascending p: a fixed order), T the same over the early partitions; ONE inverse transform of
//                           W + iT returns wet in the real and the target in the imaginary part; the valid half is kept
//   reverb_mix_kernel       one workgroup per row: both powers (fp64, fixed order), the gain, the mix, the peak, the rescale
// A spectrum of a real sequence is stored as its 1024 bins 0..1023 with the (real) Nyquist bin in the imaginary part of
// bin 0: 8 KB per partition.  Spectra pass through a workspace in HBM; a row's spectra (B = 64, 4 s, 1 s RIR: 0.5 MB of X and
// 0.13 MB of H) are re-read from L2 by the workgroups of that row.  No atomics: results repeat bit for bit, and a row's
// result does not depend on its batch-mates or on Kmax.
#include "fft_common.hpp"

namespace {

constexpr int RP = 1024;            // taps per partition = new samples per block
constexpr int RN = 2048;            // transform size
constexpr int RLOG = 11;
constexpr int RMAXTAPS = 65536;

struct ReverbWs {
    cpx* tw;                        // [RN / 2]
    cpx* H;                         // [B][nP + 1][RP]; slot nP: the early target's cut partition
    cpx* X;                         // [B][nJ][RP]
};

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

__global__ __launch_bounds__(256) void reverb_twiddle_kernel(cpx* tw) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < RN / 2) {
        double s, c;
        sincospi(2.0 * (double)t / (double)RN, &s, &c);
        tw[t] = make_float2((float)c, (float)-s);
    }
}

// half spectra of the two real sequences in Z -> dst0 (and dst1 when given)
__device__ __forceinline__ void store_half_spectra(const cpx* Z, cpx* __restrict__ dst0, cpx* __restrict__ dst1) {
    for (int k = threadIdx.x; k < RP; k += 256) {
        cpx A, Bq;
        split_pair(Z, k, RN, A, Bq);
        if (k == 0) {
            cpx An, Bn;
            split_pair(Z, RN / 2, RN, An, Bn);
            A.y = An.x;
            Bq.y = Bn.x;
        }
        dst0[k] = A;
        if (dst1) dst1[k] = Bq;
    }
}

// grid (nJ2 + nP2 + 1, B): x < nJ2 signal windows 2x, 2x+1; then RIR partitions 2q, 2q+1; the last one the early cut
__global__ __launch_bounds__(256) void reverb_spectra_kernel(const float* __restrict__ clean, const float* __restrict__ rir,
                                                             const int* __restrict__ rir_len, ReverbWs ws, int early, int L,
                                                             int Kmax, int nJ, int nP) {
    __shared__ cpx sa[RN], sb[RN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int K = min(max(rir_len[b], 0), Kmax);
    if (K == 0) return;                                       // the row does not reverberate: nothing reads its spectra
    const int nJ2 = ceil_div(nJ, 2), nP2 = ceil_div(nP, 2);
    int bx = blockIdx.x;
    if (bx < nJ2) {
        const int j = 2 * bx;
        const float* x = clean + (size_t)b * L;
        const long long s0 = ((long long)j - 1) * RP;         // window j = samples [s0, s0 + 2048), window j+1 = RP later
        for (int i = tid; i < RN; i += 256) {
            const long long s = s0 + i;
            const float re = (s >= 0 && s < L) ? x[s] : 0.f;
            const float im = (j + 1 < nJ && s + RP < L) ? x[s + RP] : 0.f;
            sa[i] = make_float2(re, im);
        }
        const cpx* Z = fft_lds_t<RLOG, false>(sa, sb, ws.tw);
        cpx* d = ws.X + ((size_t)b * nJ + j) * RP;
        store_half_spectra(Z, d, j + 1 < nJ ? d + RP : nullptr);
        return;
    }
    bx -= nJ2;
    const float* h = rir + (size_t)b * Kmax;
    cpx* Hb = ws.H + (size_t)b * (nP + 1) * RP;
    const int nPb = ceil_div(K, RP);
    if (bx < nP2) {
        const int p = 2 * bx;
        if (p >= nPb) return;
        for (int i = tid; i < RP; i += 256) {                 // taps at or beyond K are padding, never data
            const int t0 = p * RP + i, t1 = t0 + RP;
            sa[i] = make_float2(t0 < K ? h[t0] : 0.f, t1 < K ? h[t1] : 0.f);
            sa[i + RP] = make_float2(0.f, 0.f);
        }
        const cpx* Z = fft_lds_t<RLOG, false>(sa, sb, ws.tw);
        cpx* d = Hb + (size_t)p * RP;
        store_half_spectra(Z, d, p + 1 < nPb ? d + RP : nullptr);
        return;
    }
    const int Ee = min(early, K);
    if (Ee <= 0) return;
    const int pe = (Ee - 1) / RP;                             // the partition the early window ends in
    for (int i = tid; i < RP; i += 256) {
        const int t0 = pe * RP + i;
        sa[i] = make_float2(t0 < Ee ? h[t0] : 0.f, 0.f);
        sa[i + RP] = make_float2(0.f, 0.f);
    }
    const cpx* Z = fft_lds_t<RLOG, false>(sa, sb, ws.tw);
    store_half_spectra(Z, Hb + (size_t)nP * RP, nullptr);
}

// product of two packed half spectra at bin k (bin 0 carries DC in .x and Nyquist in .y, both real)
__device__ __forceinline__ cpx hmul(cpx x, cpx h, bool bin0) {
    return bin0 ? make_float2(x.x * h.x, x.y * h.y) : cmul(x, h);
}

// grid (nJ, B)
__global__ __launch_bounds__(256) void reverb_conv_kernel(const float* __restrict__ clean, const int* __restrict__ rir_len,
                                                          ReverbWs ws, int early, float* __restrict__ wet,
                                                          float* __restrict__ target, int L, int Kmax, int nJ, int nP) {
    __shared__ cpx sa[RN], sb[RN];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const int K = rir_len ? min(max(rir_len[b], 0), Kmax) : 0;
    const size_t row = (size_t)b * L;
    const int n0 = j * RP, n1 = min(n0 + RP, L);
    const int Ee = min(early, K);
    if (K == 0 || Ee <= 0) {                                  // the dry signal, bit for bit
        for (int n = n0 + tid; n < n1; n += 256) {
            const float v = clean[row + n];
            if (K == 0) wet[row + n] = v;
            target[row + n] = v;
        }
        if (K == 0) return;
    }
    const int nPb = ceil_div(K, RP);
    const int pe = Ee > 0 ? (Ee - 1) / RP : -1;
    const cpx* Hb = ws.H + (size_t)b * (nP + 1) * RP;
    const cpx* Xb = ws.X + (size_t)b * nJ * RP;
    cpx W[4], T[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) W[q] = T[q] = make_float2(0.f, 0.f);
    const int pend = min(nPb - 1, j);
    for (int p = 0; p <= pend; ++p) {
        const cpx* Xp = Xb + (size_t)(j - p) * RP;
        const cpx* Hp = Hb + (size_t)p * RP;
        const cpx* He = Hb + (size_t)nP * RP;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = tid + 256 * q;
            const cpx x = Xp[k];
            const cpx w = hmul(x, Hp[k], k == 0);
            W[q].x += w.x; W[q].y += w.y;
            if (p < pe) { T[q].x += w.x; T[q].y += w.y; }
            else if (p == pe) {
                const cpx e = hmul(x, He[k], k == 0);
                T[q].x += e.x; T[q].y += e.y;
            }
        }
    }
    // full spectrum of wet + i tgt from the two Hermitian halves
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = tid + 256 * q;
        if (k == 0) {
            sa[0] = make_float2(W[q].x, T[q].x);
            sa[RN / 2] = make_float2(W[q].y, T[q].y);
        } else {
            sa[k] = make_float2(W[q].x - T[q].y, W[q].y + T[q].x);
            sa[RN - k] = make_float2(W[q].x + T[q].y, T[q].x - W[q].y);
        }
    }
    const cpx* z = fft_lds_t<RLOG, true>(sa, sb, ws.tw);
    const float sc = 1.f / (float)RN;
    for (int n = n0 + tid; n < n1; n += 256) {
        const cpx v = z[RP + (n - n0)];                       // overlap-save: the second half is free of wrap-around
        wet[row + n] = v.x * sc;
        if (Ee > 0) target[row + n] = v.y * sc;
    }
}

// grid B; noisy holds wet on entry
__global__ __launch_bounds__(256) void reverb_mix_kernel(float* __restrict__ noisy, float* __restrict__ target,
                                                         const float* __restrict__ noise, const float* __restrict__ snr_db,
                                                         float peak, int L) {
    __shared__ double red[256];
    __shared__ float mx[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float* y = noisy + (size_t)b * L;
    float* t = target + (size_t)b * L;
    const float* v = noise ? noise + (size_t)b * L : nullptr;
    float g = 1.f;
    if (v && snr_db) {
        double ps = 0.0, pv = 0.0;
        for (int n = tid; n < L; n += 256) {
            const double a = y[n], c = v[n];
            ps += a * a;
            pv += c * c;
        }
        ps = block_sum_f64(ps, red) / (double)L;
        pv = block_sum_f64(pv, red) / (double)L;
        if (ps >= 1e-20 && pv >= 1e-20) g = (float)sqrt(ps / (pv * pow(10.0, (double)snr_db[b] / 10.0)));
    }
    float m = 0.f;
    for (int n = tid; n < L; n += 256) {
        float o = y[n];
        if (v) { o += g * v[n]; y[n] = o; }
        m = fmaxf(m, fabsf(o));
    }
    if (!(peak > 0.f)) return;
    mx[tid] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) mx[tid] = fmaxf(mx[tid], mx[tid + s]);
        __syncthreads();
    }
    m = mx[0];
    if (!(m > peak)) return;
    const float sc = peak / m;
    for (int n = tid; n < L; n += 256) {                      // every thread rescales the samples it wrote itself
        y[n] *= sc;
        t[n] *= sc;
    }
}

struct ReverbLayout { size_t tw, H, X, total; int nJ, nP; };

ReverbLayout reverb_layout(int B, int L, int Kmax) {
    ReverbLayout r;
    r.nJ = ceil_div(L, RP);
    r.nP = ceil_div(Kmax, RP);
    r.tw = 0;
    r.H = r.tw + (size_t)(RN / 2) * sizeof(cpx);
    r.X = r.H + (size_t)B * (r.nP + 1) * RP * sizeof(cpx);
    r.total = r.X + (size_t)B * r.nJ * RP * sizeof(cpx);
    return r;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

extern "C" size_t trunet_reverb_workspace_bytes(int B, int L, int Kmax) {
    if (B <= 0 || L <= 0 || Kmax <= 0 || Kmax > RMAXTAPS) return 0;
    return reverb_layout(B, L, Kmax).total;
}

extern "C" int trunet_reverb_mix(const float* clean, const float* noise, const float* rir, const int* rir_len,
                                 const float* snr_db, int early_taps, float peak, float* noisy, float* target, void* ws,
                                 size_t ws_bytes, int B, int L, int Kmax, void* stream) {
    if (!clean || !noisy || !target || B <= 0 || L <= 0 || early_taps < 0) return TRUNET_EINVAL;
    if (rir ? (Kmax <= 0 || !rir_len) : Kmax < 0) return TRUNET_EINVAL;
    if (Kmax > RMAXTAPS) return TRUNET_ENOTSUP;
    if ((size_t)B > ((size_t)1 << 16) - 1) return TRUNET_EINVAL;                      // rows ride gridDim.y
    const size_t bytes = (size_t)B * L * sizeof(float);
    if (overlap(noisy, bytes, target, bytes) || overlap(noisy, bytes, clean, bytes) || overlap(target, bytes, clean, bytes) ||
        overlap(noisy, bytes, noise, bytes) || overlap(target, bytes, noise, bytes))
        return TRUNET_EINVAL;
    ReverbWs w = {nullptr, nullptr, nullptr};
    ReverbLayout lay = {0, 0, 0, 0, ceil_div(L, RP), 0};
    if (rir) {
        lay = reverb_layout(B, L, Kmax);
        if (!ws || ws_bytes < lay.total || ((uintptr_t)ws & 7)) return TRUNET_EINVAL;
        const size_t rbytes = (size_t)B * Kmax * sizeof(float);
        if (overlap(ws, lay.total, noisy, bytes) || overlap(ws, lay.total, target, bytes) ||
            overlap(ws, lay.total, clean, bytes) || overlap(ws, lay.total, noise, bytes) || overlap(ws, lay.total, rir, rbytes) ||
            overlap(rir, rbytes, noisy, bytes) || overlap(rir, rbytes, target, bytes))
            return TRUNET_EINVAL;
        w.tw = (cpx*)((char*)ws + lay.tw);
        w.H = (cpx*)((char*)ws + lay.H);
        w.X = (cpx*)((char*)ws + lay.X);
    }
    hipStream_t st = (hipStream_t)stream;
    if (rir) {
        hipLaunchKernelGGL(reverb_twiddle_kernel, dim3(RN / 2 / 256), dim3(256), 0, st, w.tw);
        hipLaunchKernelGGL(reverb_spectra_kernel, dim3(ceil_div(lay.nJ, 2) + ceil_div(lay.nP, 2) + 1, B), dim3(256), 0, st,
                           clean, rir, rir_len, w, early_taps, L, Kmax, lay.nJ, lay.nP);
    }
    hipLaunchKernelGGL(reverb_conv_kernel, dim3(lay.nJ, B), dim3(256), 0, st, clean, rir ? rir_len : nullptr, w, early_taps,
                       noisy, target, L, Kmax, lay.nJ, lay.nP);
    if (noise || peak > 0.f)
        hipLaunchKernelGGL(reverb_mix_kernel, dim3(B), dim3(256), 0, st, noisy, target, noise, snr_db, peak, L);
    return trunet_launch_status();
}
