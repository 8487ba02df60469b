// LDS FFT device code shared by fft.hip (features, iSTFT, losses) and metrics.hip (STOI / ESTOI front end).
#pragma once
#include "common.hpp"

namespace {

typedef float2 cpx;

__device__ __forceinline__ cpx cmul(cpx a, cpx b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cpx cconj(cpx a) { return make_float2(a.x, -a.y); }

// In-LDS Stockham FFT (fft.hip: fft_lds) with the size as a COMPILE-TIME constant (n = 2^LOGN, 256 threads): every stage's butterfly count per thread,
// twiddle stride and index masks fold to constants and the stage loop unrolls.  The STFT-loss kernels run ~400 wave
// instructions per block and are instruction-issue-bound (82k blocks x 4 waves at n = 512: the generic form, with its
// runtime `quarter / ns` divisions and masked index arithmetic, is most of that); round 3.
// tw[t] = exp(-2*pi*i*t/n), t < n/2; INV => conjugated twiddles (unnormalised); returns the buffer holding the result.
template <int LOGN, bool INV>
__device__ __forceinline__ cpx* fft_lds_t(cpx* a, cpx* b, const cpx* __restrict__ tw) {
    constexpr int n = 1 << LOGN, half = n >> 1, quarter = n >> 2;
    cpx* x = a;
    cpx* y = b;
    if constexpr (LOGN & 1) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < (half + 255) / 256; ++it) {
            const int j = threadIdx.x + 256 * it;
            if (half >= 256 || j < half) {
                const cpx u = x[j], v = x[j + half];
                y[2 * j] = make_float2(u.x + v.x, u.y + v.y);
                y[2 * j + 1] = make_float2(u.x - v.x, u.y - v.y);
            }
        }
        cpx* t = x; x = y; y = t;
    }
#pragma unroll
    for (int s = (LOGN & 1); s < LOGN; s += 2) {
        const int ns = 1 << s;                       // constant after unrolling
        const int tstep = quarter >> s;
        __syncthreads();
#pragma unroll
        for (int it = 0; it < (quarter + 255) / 256; ++it) {
            const int j = threadIdx.x + 256 * it;
            if (quarter >= 256 || j < quarter) {
                const int k = j & (ns - 1);
                const int t1 = k * tstep;
                cpx w1 = tw[t1], w2 = tw[2 * t1];
                const int t3 = 3 * t1;
                cpx w3 = tw[t3 >= half ? t3 - half : t3];
                if (t3 >= half) { w3.x = -w3.x; w3.y = -w3.y; }
                if (INV) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
                const cpx u0 = x[j];
                const cpx u1 = cmul(w1, x[j + quarter]);
                const cpx u2 = cmul(w2, x[j + 2 * quarter]);
                const cpx u3 = cmul(w3, x[j + 3 * quarter]);
                const cpx v0 = make_float2(u0.x + u2.x, u0.y + u2.y);
                const cpx v1 = make_float2(u0.x - u2.x, u0.y - u2.y);
                const cpx v2 = make_float2(u1.x + u3.x, u1.y + u3.y);
                const cpx d = make_float2(u1.x - u3.x, u1.y - u3.y);
                const cpx v3 = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);
                const int j0 = ((j - k) << 2) + k;
                y[j0] = make_float2(v0.x + v2.x, v0.y + v2.y);
                y[j0 + ns] = make_float2(v1.x + v3.x, v1.y + v3.y);
                y[j0 + 2 * ns] = make_float2(v0.x - v2.x, v0.y - v2.y);
                y[j0 + 3 * ns] = make_float2(v1.x - v3.x, v1.y - v3.y);
            }
        }
        cpx* t = x; x = y; y = t;
    }
    __syncthreads();
    return x;
}

// the two real sequences a, b of z = a + j b: A[k] = (Z[k] + conj Z[n-k]) / 2, B[k] = (Z[k] - conj Z[n-k]) / (2j)
__device__ __forceinline__ void split_pair(const cpx* Z, int k, int n, cpx& A, cpx& B) {
    const cpx zk = Z[k];
    const cpx zn = cconj(Z[(n - k) & (n - 1)]);
    A = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y + zn.y));
    // (zk - zn) / (2j) = (-j/2) (zk - zn)
    B = make_float2(0.5f * (zk.y - zn.y), -0.5f * (zk.x - zn.x));
}

}  // namespace
