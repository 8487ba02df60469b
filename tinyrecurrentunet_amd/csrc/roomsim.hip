// Room simulation on the GPU: one room impulse response (RIR) per row of a batch, by the image-source method (ISM) up to a
// crossover tap n_c and a stochastic diffuse tail after it (float64 statement: tests/roomsim_ref.py).
// A row is 18 floats: Lx Ly Lz | sx sy sz | rx ry rz | bx0 bx1 by0 by1 bz0 bz1 | rt60 | seed_lo seed_hi (16-bit halves).
//   K_b   = clamp(round(min(rt60, max_rir_sec) fs), 1, Kmax)
//   ISM   0 <= n < min(n_c, K_b): for p = (q, j, k) in {0,1}^3 and m in Z^3 the image I = ((1-2q) sx + 2 mx Lx, ...),
//         d = |I - r|, d0 = |s - r|, tau = (d - d0) fs / c, gain = bx0^|mx-q| bx1^|mx| ... bz1^|mz| d0 / d,
//         h[n] += gain 0.5 (1 + cos(2 pi (n - tau) / tw)) sinc(n - tau)   for |n - tau| < tw / 2
//   tail  n_c <= n < K_b: sigma_c g(seed, n) exp(-6.9078 (n - n_c + W/2) / (rt60 fs)), W = max(round(0.010 fs), 1),
//         sigma_c^2 = mean h[n]^2 over max(n_c - W, 0) <= n < n_c, g a standard normal from an integer hash of (seed, n)
//   zeros K_b <= n < Kmax; a malformed row (see rs_load) is all zeros with rir_len = 0
//
// rir_ism_kernel   one workgroup per (row, segment of RS_SEG taps).  The segment lives in LDS as 64-bit fixed-point
//                  accumulators (resolution 2^-40): integer addition is associative, so the LDS atomics may land in any order
//                  and the taps still repeat bit for bit.  A term is a pure function of (image, n), never of the lane or the
//                  segment that computes it, so a row does not depend on its batch-mates or on Kmax either.
//                  Work item = (mx, my, q, j, k); the mz range whose distance shell can reach the segment is solved from
//                  d_lo^2 - rho^2 < dz^2 < d_hi^2 - rho^2 (one step of slack on each end, the exact test is per tap).
//                  Positions, d and tau are fp64, the taps fp32: sin(pi (n - tau)) = -(-1)^k sin(pi frac) with n = n0 + k,
//                  and the window's cosine comes from a table of cos / sin(2 pi k / tw) by angle addition.
// rir_tail_kernel  sigma_c in fp64 in a fixed order, the tail, the zero padding and rir_len.
// Every loop bound is a compile-time constant or a host argument checked against a cap: image orders are clamped to
// RS_NORD per axis, so no bit pattern in a row lengthens a loop.
#include "common.hpp"

namespace {

constexpr int RS_ROW = 18;
constexpr int RS_SEG = 512;               // taps per workgroup of the ISM kernel
constexpr int RS_TAILSEG = 1024;          // taps per workgroup of the tail kernel
constexpr int RS_MAX_NC = 8192;           // cap on the ISM span in taps
constexpr int RS_MAX_TW = 129;
constexpr int RS_MAX_K = 65536;           // trunet_reverb_mix's limit
constexpr float RS_MIN_DIM = 2.f;         // metres
constexpr double RS_MAX_SPAN_M = 360.0;   // cap on (n_c + tw/2 + 1) c / fs: 8192 taps at 8 kHz and 343 m/s are 354 m
// |x_I - r| > 2 L (|m| - 1) for s, r inside the room, so an image within d_hi = d0 + span has |m| < 1 + d_hi / (2 L):
// 1 + 360 / 4 = 91 at the 2 m minimum, and 96 leaves d0 <= 20 m along a 2 m axis.  Beyond that the clamp drops images.
constexpr int RS_NORD = 96;
constexpr float RS_FIX = 1099511627776.f; // 2^40
constexpr double RS_UNFIX = 1.0 / 1099511627776.0;

struct Room {
    double L[3], s[3], r[3], d0, rt60;
    uint32_t seed;
    int K;                                // K_b
};

__host__ __device__ inline int rs_ceil_div(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ double rs_norm3(double dx, double dy, double dz) {
    return sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
}

// lowbias32 (two multiply-xorshift rounds); the generator's integer part, restated bit for bit in tests/roomsim_ref.py
__device__ __forceinline__ uint32_t rs_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t rs_word(uint32_t seed, uint32_t key, uint32_t ctr) {
    return rs_mix(rs_mix(ctr ^ key) + seed);
}

// decode and validate a row; false: malformed (NaN, Inf, a dimension below 2 m, a point not strictly inside, |beta| > 1,
// rt60 <= 0, seed halves that are not integers in [0, 65535], source and microphone closer than 1 mm) or all zero
__device__ bool rs_load(const float* __restrict__ p, float fs, float max_rir_sec, int Kmax, Room& R) {
    float v[RS_ROW];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < RS_ROW; ++i) {
        v[i] = p[i];
        ok = ok && (fabsf(v[i]) <= 3.0e38f);                  // false for NaN and Inf
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        ok = ok && v[a] >= RS_MIN_DIM && v[3 + a] > 0.f && v[3 + a] < v[a] && v[6 + a] > 0.f && v[6 + a] < v[a];
        R.L[a] = v[a]; R.s[a] = v[3 + a]; R.r[a] = v[6 + a];
    }
#pragma unroll
    for (int w = 0; w < 6; ++w) ok = ok && fabsf(v[9 + w]) <= 1.f;
    ok = ok && v[15] > 0.f;
    ok = ok && v[16] >= 0.f && v[16] <= 65535.f && v[16] == floorf(v[16]);
    ok = ok && v[17] >= 0.f && v[17] <= 65535.f && v[17] == floorf(v[17]);
    if (!ok) return false;
    R.rt60 = v[15];
    R.seed = ((uint32_t)v[17] << 16) | (uint32_t)v[16];
    R.d0 = rs_norm3(R.s[0] - R.r[0], R.s[1] - R.r[1], R.s[2] - R.r[2]);
    if (!(R.d0 >= 1e-3)) return false;
    const double k = rint((double)fminf(v[15], max_rir_sec) * (double)fs);
    R.K = (int)fmin(fmax(k, 1.0), (double)Kmax);
    return true;
}

// double -> int inside [-lim, lim]
__device__ __forceinline__ int rs_clampi(double x, int lim) { return (int)fmin(fmax(x, (double)-lim), (double)lim); }

// grid (ceil(min(n_c, Kmax) / RS_SEG), B)
__global__ __launch_bounds__(256) void rir_ism_kernel(const float* __restrict__ rooms, float* __restrict__ rir, int Kmax,
                                                      float fs, float c, int n_c, int tw, float max_rir_sec) {
    __shared__ unsigned long long acc[RS_SEG];
    __shared__ float pw[6][RS_NORD + 2];
    __shared__ float ck[RS_MAX_TW], sk[RS_MAX_TW];
    const int b = blockIdx.y, tid = threadIdx.x;
    Room R;
    if (!rs_load(rooms + (size_t)b * RS_ROW, fs, max_rir_sec, Kmax, R)) return;     // the tail kernel writes the zeros
    const int n_ism = min(n_c, R.K);
    const int n_a = blockIdx.x * RS_SEG;
    if (n_a >= n_ism) return;
    const int n_b = min(n_a + RS_SEG, n_ism);
    const int half = tw / 2;                                    // tw is odd: taps n0 - half .. n0 + half
    for (int i = tid; i < RS_SEG; i += 256) acc[i] = 0ull;
    for (int i = tid; i < 6 * (RS_NORD + 2); i += 256) {        // beta^e by e multiplications in fp64: one fixed order
        const int w = i / (RS_NORD + 2), e = i % (RS_NORD + 2);
        const double bw = rooms[(size_t)b * RS_ROW + 9 + w];
        double y = 1.0;
        for (int t = 0; t < e; ++t) y *= bw;
        pw[w][e] = (float)y;
    }
    for (int i = tid; i < tw; i += 256) {
        double s_, c_;
        sincospi(2.0 * (double)(i - half) / (double)tw, &s_, &c_);
        sk[i] = (float)s_;
        ck[i] = (float)c_;
    }
    __syncthreads();

    const double spm = (double)fs / (double)c;                  // samples per metre
    const double d_hi = R.d0 + (double)(n_b + half + 1) / spm;  // images that can reach the segment: d_lo < d < d_hi
    const double d_lo = R.d0 + (double)(n_a - half - 2) / spm;
    const int Nx = rs_clampi(d_hi / (2.0 * R.L[0]) + 1.0, RS_NORD);
    const int Ny = rs_clampi(d_hi / (2.0 * R.L[1]) + 1.0, RS_NORD);
    const int nx = 2 * Nx + 1, ny = 2 * Ny + 1;
    const int items = nx * ny * 8;                              // <= 193 * 193 * 8
    const double twoLx = 2.0 * R.L[0], twoLy = 2.0 * R.L[1], twoLz = 2.0 * R.L[2];
    const float two_over_tw = 2.f / (float)tw;
    for (int it = tid; it < items; it += 256) {
        const int q = it & 1, j = (it >> 1) & 1, k = (it >> 2) & 1;
        const int col = it >> 3;
        const int mx = col % nx - Nx, my = col / nx - Ny;
        const double dx = ((q ? -R.s[0] : R.s[0]) - R.r[0]) + twoLx * (double)mx;
        const double dy = ((j ? -R.s[1] : R.s[1]) - R.r[1]) + twoLy * (double)my;
        const double rho2 = fma(dy, dy, dx * dx);
        const double hi2 = d_hi * d_hi - rho2;
        if (!(hi2 > 0.0)) continue;
        const double a = (k ? -R.s[2] : R.s[2]) - R.r[2];
        const double zhi = sqrt(hi2);
        const int m_a = rs_clampi(ceil((-zhi - a) / twoLz) - 1.0, RS_NORD);
        const int m_b = rs_clampi(floor((zhi - a) / twoLz) + 1.0, RS_NORD);
        int g_a = 1, g_b = 0;                                   // the orders strictly inside the shell: skipped
        const double lo2 = d_lo * d_lo - rho2;
        if (d_lo > 0.0 && lo2 > 0.0) {
            const double zlo = sqrt(lo2);
            g_a = rs_clampi(ceil((-zlo - a) / twoLz) + 1.0, RS_NORD + 1);
            g_b = rs_clampi(floor((zlo - a) / twoLz) - 1.0, RS_NORD + 1);
        }
        const float gxy = pw[0][abs(mx - q)] * pw[1][abs(mx)] * pw[2][abs(my - j)] * pw[3][abs(my)];
        if (gxy == 0.f) continue;
        for (int mz = m_a; mz <= m_b; ++mz) {
            if (mz >= g_a && mz <= g_b) { mz = g_b; continue; }
            const double dz = a + twoLz * (double)mz;
            const double d = sqrt(fma(dz, dz, rho2));
            const double tau = (d - R.d0) * spm;
            const double n0 = rint(tau);
            if (!(n0 > (double)(n_a - half - 1) && n0 < (double)(n_b + half))) continue;
            const int in0 = (int)n0;
            const int k_lo = max(-half, n_a - in0), k_hi = min(half, n_b - 1 - in0);
            if (k_lo > k_hi) continue;
            const float gain = gxy * pw[4][abs(mz - k)] * pw[5][abs(mz)] * (float)(R.d0 / d);
            if (gain == 0.f) continue;
            const float f = (float)(tau - n0);                  // in [-0.5, 0.5]
            float S, C_, sf, cf;
            sincospif(f, &S, &C_);
            sincospif(two_over_tw * f, &sf, &cf);
            for (int kk = k_lo; kk <= k_hi; ++kk) {             // <= tw <= 129 taps, all inside [n_a, n_b)
                const float t = (float)kk - f;
                const float w = 0.5f * (1.f + ck[kk + half] * cf + sk[kk + half] * sf);
                const float sinc = (t == 0.f) ? 1.f : ((kk & 1) ? S : -S) / (3.14159265358979f * t);
                const float val = gain * w * sinc;
                const long long qv = __float2ll_rn(val * RS_FIX);
                atomicAdd(&acc[in0 + kk - n_a], (unsigned long long)qv);
            }
        }
    }
    __syncthreads();
    float* h = rir + (size_t)b * Kmax;
    for (int n = n_a + tid; n < n_b; n += 256) h[n] = (float)((double)(long long)acc[n - n_a] * RS_UNFIX);
}

// grid (ceil(Kmax / RS_TAILSEG), B); runs after rir_ism_kernel on the same stream
__global__ __launch_bounds__(256) void rir_tail_kernel(const float* __restrict__ rooms, float* __restrict__ rir,
                                                       int32_t* __restrict__ rir_len, int Kmax, float fs, int n_c,
                                                       float max_rir_sec) {
    __shared__ double red[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    Room R;
    const bool ok = rs_load(rooms + (size_t)b * RS_ROW, fs, max_rir_sec, Kmax, R);
    const int K = ok ? R.K : 0;
    if (blockIdx.x == 0 && tid == 0) rir_len[b] = K;
    const int n_ism = min(n_c, K);
    const int n_a = blockIdx.x * RS_TAILSEG, n_b = min(n_a + RS_TAILSEG, Kmax);
    float* h = rir + (size_t)b * Kmax;
    const bool tail = K > n_c && n_b > n_c && n_a < K;          // uniform over the workgroup
    const int W = max((int)rint(0.010 * (double)fs), 1);
    float sigma = 0.f;
    uint32_t key = 0;
    double rate = 0.0;
    if (tail) {
        const int w0 = max(n_c - W, 0);                         // n_c <= RS_MAX_NC taps at the most
        double s2 = 0.0;
        for (int n = w0 + tid; n < n_c; n += 256) {
            const double x = h[n];
            s2 = fma(x, x, s2);
        }
        s2 = block_sum_f64(s2, red);
        sigma = (float)sqrt(s2 / (double)(n_c - w0));
        key = rs_mix(R.seed + 0x9E3779B9U);
        rate = -6.9078 / (R.rt60 * (double)fs);
    }
    for (int n = n_a + tid; n < n_b; n += 256) {
        if (n < n_ism) continue;                                // an image-source tap
        float val = 0.f;
        if (n >= n_c && n < K) {
            const uint32_t wa = rs_word(R.seed, key, 2u * (uint32_t)n), wb = rs_word(R.seed, key, 2u * (uint32_t)n + 1u);
            const float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-08f;     // (0, 1]
            const float u2 = (float)(wb >> 8) * 5.9604644775390625e-08f;            // [0, 1)
            const float g = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
            const float env = expf((float)(rate * ((double)(n - n_c) + 0.5 * (double)W)));
            val = sigma * g * env;
        }
        h[n] = val;
    }
}

constexpr size_t RS_WS_BYTES = 256;       // reserved: the accumulators live in LDS, nothing passes through HBM

}  // namespace

extern "C" size_t trunet_rir_ism_workspace_bytes(int B, int Kmax) {
    if (B <= 0 || Kmax <= 0 || Kmax > RS_MAX_K) return 0;
    return RS_WS_BYTES;
}

extern "C" int trunet_rir_ism(const float* rooms, int row_floats, float* rir, int32_t* rir_len, int B, int Kmax, float fs,
                              float c, int n_c, int tw, float max_rir_sec, void* ws, size_t ws_bytes, void* stream) {
    if (!rooms || !rir || !rir_len || row_floats != RS_ROW || B <= 0 || Kmax <= 0 || n_c < 1 || tw < 1) return TRUNET_EINVAL;
    if (!(fs > 0.f) || !(c > 0.f) || !(max_rir_sec > 0.f) || !(fs <= 3.0e38f) || !(c <= 3.0e38f) || !(max_rir_sec <= 3.0e38f))
        return TRUNET_EINVAL;
    if ((size_t)B > ((size_t)1 << 16) - 1) return TRUNET_EINVAL;                      // rows ride gridDim.y
    if (Kmax > RS_MAX_K || n_c > RS_MAX_NC || tw > RS_MAX_TW || (tw & 1) == 0) return TRUNET_ENOTSUP;
    if ((double)(n_c + tw / 2 + 1) * (double)c / (double)fs > RS_MAX_SPAN_M) return TRUNET_ENOTSUP;
    if (!ws || ws_bytes < RS_WS_BYTES) return TRUNET_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rir_ism_kernel, dim3(rs_ceil_div(n_c < Kmax ? n_c : Kmax, RS_SEG), B), dim3(256), 0, st, rooms, rir,
                       Kmax, fs, c, n_c, tw, max_rir_sec);
    hipLaunchKernelGGL(rir_tail_kernel, dim3(rs_ceil_div(Kmax, RS_TAILSEG), B), dim3(256), 0, st, rooms, rir, rir_len, Kmax,
                       fs, n_c, max_rir_sec);
    return trunet_launch_status();
}
