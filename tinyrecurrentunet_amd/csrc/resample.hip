// Rational resampling of B utterances of any lengths, packed back to back (resample.py):
//   y[m] = p sum_n h[m q - n p + half] x[n],  m < ceil(L_b p / q),  h = 2 half + 1 taps, zero outside
// (scipy.signal.resample_poly(x, p, q, window=h)).  Unlike metrics.hip's resample_poly_kernel (STOI's 10 kHz resampler,
// one global load per tap) a workgroup owns one tile of `tile` consecutive outputs of ONE utterance, counted from that
// utterance's first output, and stages the tile's input span in LDS once: zeros outside [0, L_b), so the tap loop has no
// bounds test and no global load of a sample.  The taps come phase-major, table[r][k] = h[r + k p] in rows of
// Kp = round_up(K, 4) floats (zero padded): the K taps of output m (r = (m q + half) % p, n = (m q + half) / p - k) are
// one contiguous row, read four at a time from LDS (TAPS_LDS) or from L2.  Every output accumulates in fp32 with k
// ascending; tiles do not depend on the batch, so an utterance's result is bit for bit independent of its batch-mates.
// A span longer than RS_SPAN_MAX floats (only ratios far below 1: q / p above 16 or so) is staged in windows of
// RS_SPAN_MAX, highest samples first, which keeps k ascending.
#include "common.hpp"

namespace {

constexpr int RS_MAX_RATIO = 640;
constexpr int RS_MAX_ZEROS = 32;                 // half <= 32 max(p, q)
constexpr int RS_MAX_TILE = 4096;
constexpr int RS_SPAN_MAX = 4608;                // floats of input staged per window (18 KiB)
constexpr int RS_STAGE = 6;                      // loads a thread keeps in flight while it stages
constexpr int RS_TAPS_LDS_MAX = 16384;           // floats of the tap table that may live in LDS (64 KiB)

// largest b in [0, B) with off[b] <= v (metrics.hip's utt_find)
__device__ __forceinline__ int rs_find(const int64_t* __restrict__ off, int B, int64_t v) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// grid (total_tiles, nsig); plane y of in / out starts at y * nIn / y * nOut.  LDS: span floats of samples, then the table.
template <bool TAPS_LDS>
__global__ __launch_bounds__(256) void resample_rational_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                const int64_t* __restrict__ io,
                                                                const int64_t* __restrict__ oo,
                                                                const int64_t* __restrict__ to,
                                                                const float* __restrict__ table, int half, int K, int p,
                                                                int q, int tile, int span, int B, int64_t nIn,
                                                                int64_t nOut, int64_t nTiles) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int Kp = (K + 3) & ~3;
    float* xs = rs_lds;
    const float* tab = table;
    if (TAPS_LDS) {
        float* ts = rs_lds + span;                     // span is a multiple of 4: rows stay 16-byte aligned
        const f32x4* src = reinterpret_cast<const f32x4*>(table);
        f32x4* dst = reinterpret_cast<f32x4*>(ts);
        const int n4 = p * (Kp >> 2);
        for (int i = threadIdx.x; i < n4; i += 256 * 4) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i + 256 * u < n4 ? src[i + 256 * u] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i + 256 * u < n4) dst[i + 256 * u] = v[u];
        }
        tab = ts;
    }
    const int b = rs_find(to, B, (int64_t)blockIdx.x);
    const int64_t i0 = io[b], i1 = io[b + 1], o0 = oo[b], o1 = oo[b + 1], t0 = to[b], t1 = to[b + 1];
    // workgroup-uniform: an utterance whose offsets contradict each other is skipped
    if (i0 < 0 || i1 > nIn || i1 < i0 || o0 < 0 || o1 > nOut || o1 - o0 != ((i1 - i0) * p + q - 1) / q || t0 < 0 ||
        t1 > nTiles || t1 - t0 != (o1 - o0 + tile - 1) / tile || (int64_t)blockIdx.x < t0 || (int64_t)blockIdx.x >= t1)
        return;
    const int64_t len = i1 - i0, M = o1 - o0;
    const int64_t m0 = ((int64_t)blockIdx.x - t0) * tile;
    const int64_t mlast = (m0 + tile < M ? m0 + tile : M) - 1;
    const float* x = in + (size_t)blockIdx.y * nIn + i0;
    // samples the tile reads: n_lo .. n_hi, n_hi the first sample of its last output, n_lo the last of its first.
    // c0 = m0 q + half = nmax0 p + r0; output m0 + j then has c = c0 + j q, so 32-bit arithmetic does per output
    const int64_t c0 = m0 * q + half;
    const int64_t nmax0 = c0 / p;
    const int r0 = (int)(c0 - nmax0 * p);
    const int64_t n_hi = (mlast * q + half) / p;
    const int64_t n_lo = nmax0 - (Kp - 1);
    const int jlast = (int)(mlast - m0);
    float* y = out + (size_t)blockIdx.y * nOut + o0 + m0;

    for (int64_t top = n_hi; top >= n_lo; top -= span) {
        const int64_t w0 = top - span + 1;              // this window holds samples w0 .. top at xs[0 .. span)
        __syncthreads();                                // the table is in place / the last window has been read
        for (int i = threadIdx.x; i < span; i += 256 * RS_STAGE) {      // RS_STAGE loads in flight per thread
            float v[RS_STAGE];
#pragma unroll
            for (int u = 0; u < RS_STAGE; ++u) {
                const int64_t n = w0 + i + 256 * u;
                v[u] = (i + 256 * u < span && n >= 0 && n < len) ? x[n] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < RS_STAGE; ++u)
                if (i + 256 * u < span) xs[i + 256 * u] = v[u];
        }
        __syncthreads();
        const int d0 = (int)(nmax0 - w0);
        for (int j = threadIdx.x; j <= jlast; j += 256) {
            const unsigned c = (unsigned)j * (unsigned)q + (unsigned)r0;
            const unsigned dn = c / (unsigned)p;
            const int r = (int)(c - dn * (unsigned)p);
            const float* row = tab + r * Kp;
            const int base = d0 + (int)dn;              // xs index of tap 0's sample; tap k reads xs[base - k]
            // taps k of this output whose sample lies in the window
            const int klo = base > span - 1 ? base - (span - 1) : 0;
            const int khi = base < K - 1 ? base : K - 1;
            if (klo > khi) continue;
            float acc = klo == 0 ? 0.f : y[j];          // the running sum waits in `out` between windows
            if (klo == 0 && khi == K - 1 && base >= Kp - 1) {
                const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
#pragma unroll 4
                for (int k4 = 0; k4 < (Kp >> 2); ++k4) {
                    const f32x4 h = row4[k4];
                    const float* xp = xs + base - 4 * k4;
                    acc = fmaf(h.x, xp[0], acc);
                    acc = fmaf(h.y, xp[-1], acc);
                    acc = fmaf(h.z, xp[-2], acc);
                    acc = fmaf(h.w, xp[-3], acc);
                }
            } else {
                for (int k = klo; k <= khi; ++k) acc = fmaf(row[k], xs[base - k], acc);
            }
            y[j] = khi == K - 1 ? (float)p * acc : acc; // the last tap's window scales by p
        }
    }
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_resample_rational(const float* in, float* out, const int64_t* in_off, const int64_t* out_off,
                                        const int64_t* tile_off, const float* table, int half, int K, int p, int q,
                                        int tile, int B, int64_t total_in, int64_t total_out, int64_t total_tiles,
                                        int nsig, int taps_in_lds, void* stream) {
    if (!in || !out || !in_off || !out_off || !tile_off || !table || B < 1 || nsig < 1 || nsig > 2 || p < 1 ||
        p > RS_MAX_RATIO || q < 1 || q > RS_MAX_RATIO || taps_in_lds < 0 || taps_in_lds > 1)
        return TRUNET_EINVAL;
    const int big = p > q ? p : q;
    if (half < big || half % big != 0 || half / big > RS_MAX_ZEROS || K != (2 * half + p) / p) return TRUNET_EINVAL;
    if (tile < 256 || tile > RS_MAX_TILE || tile % 256 != 0) return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (total_in < 0 || total_out < 0 || total_tiles < 0 || total_in > lim || total_out > lim) return TRUNET_EINVAL;
    // sum ceil(L_b p / q) lies in [total_in p / q, total_in p / q + B), sum ceil(M_b / tile) likewise
    if (total_out * q < total_in * p || total_out * q >= total_in * p + (int64_t)B * q) return TRUNET_EINVAL;
    if (total_tiles * tile < total_out || total_tiles * tile >= total_out + (int64_t)B * tile) return TRUNET_EINVAL;
    const int Kp = (K + 3) & ~3;
    if (taps_in_lds && p * Kp > RS_TAPS_LDS_MAX) return TRUNET_EINVAL;
    if (total_out == 0) return TRUNET_OK;
    // the whole span of a full tile if it fits, else windows of RS_SPAN_MAX
    int64_t span = ((int64_t)(tile - 1) * q + p - 1) / p + Kp + 1;
    span = (span + 3) & ~(int64_t)3;
    if (span > RS_SPAN_MAX) span = RS_SPAN_MAX;
    const size_t lds = ((size_t)span + (taps_in_lds ? (size_t)p * Kp : 0)) * sizeof(float);
    auto kern = taps_in_lds ? resample_rational_kernel<true> : resample_rational_kernel<false>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)total_tiles, nsig), dim3(256), lds, ST, in, out, in_off, out_off, tile_off,
                       table, half, K, p, q, tile, (int)span, B, total_in, total_out, total_tiles);
    return trunet_launch_status();
}
