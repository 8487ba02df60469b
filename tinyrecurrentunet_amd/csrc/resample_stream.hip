// Stateful rational resampling of streaming sessions (resample.py: StreamResampler).  The definition and
// the per-output expression are those of resample.hip,
//   y[m] = p sum_n h[m q - n p + half] x[n]:  acc = 0, fmaf(row[k], x[nmax - k], acc) with k ascending over the
//   phase-major row table[(m q + half) % p], nmax = (m q + half) / p, then (float)p * acc, zeros outside the session,
// so that however a session is cut into packets its outputs are bit for bit those of trunet_resample_rational on the whole.
// A session that had N0 samples before the call and brings a packet of n is the LINE
//   hist[slot] (x[N0 - H, N0), H = K - 1)  ++  in[poff, poff + n)
// with zeros left of sample 0 and right of N1 = N0 + n (only a closing session's outputs reach there).  The next output
// of a session reads no sample below N0 - H: it is m = ceil((N0 p - half) / q) or later, so m q + half >= N0 p,
// nmax >= N0 and nmax - (K - 1) >= N0 - H.
// plan: (n_sess, TRUNET_RS_STREAM_INTS) int64, one record per listed session:
//   [0] slot  [1] N0  [2] poff  [3] n  [4] first output m0  [5] outputs  [6] offset in `out`  [7] closing  [8], [9] the
//   session's tiles [t0, t1) of the grid, t1 - t0 = ceil(outputs / tile).
// resample_stream_kernel: a workgroup owns one tile of consecutive outputs of ONE session, counted from m0, stages the
// tile's span of the line in LDS and runs resample.hip's tap loop; it reads hist only.  resample_stream_commit_kernel, after
// it on the same stream: one workgroup per session, hist[slot] <- the last H samples of the line, through LDS (every read
// of the old history comes before the first write).  A record whose slot, packet extent, output extent or tiles lie
// outside the extents passed in is skipped, workgroup-uniformly.
#include "common.hpp"

namespace {

constexpr int RSS_MAX_RATIO = 640;
constexpr int RSS_MAX_ZEROS = 32;
constexpr int RSS_MAX_TILE = 4096;
constexpr int RSS_SPAN_MAX = 4608;               // resample.hip: RS_SPAN_MAX
constexpr int RSS_STAGE = 6;
constexpr int RSS_TAPS_LDS_MAX = 16384;          // resample.hip: RS_TAPS_LDS_MAX
constexpr int RSS_INTS = TRUNET_RS_STREAM_INTS;
constexpr int RSS_HIST_MAX = TRUNET_RS_STREAM_MAX_HISTORY;
constexpr int64_t RSS_MAX_COUNT = (int64_t)1 << 40;      // samples of a session (resample.py: MAX_SESSION)
constexpr int64_t RSS_MAX_OUTPUT = (int64_t)1 << 50;     // its outputs, at most 640 times as many: m q + half stays inside int64

struct rss_line {
    const float* hist;       // the slot's H history samples, x[N0 - H .. N0)
    const float* pkt;        // the packet, x[N0 .. N1)
    int64_t N0, N1;
    int H;
};

// sample n of the session; zero outside [0, N1) and below what the history keeps
__device__ __forceinline__ float rss_sample(const rss_line& s, int64_t n) {
    if (n < 0 || n >= s.N1) return 0.f;
    if (n >= s.N0) return s.pkt[n - s.N0];
    const int64_t back = s.N0 - n;               // 1: the newest history sample
    return back <= s.H ? s.hist[s.H - back] : 0.f;
}

// largest b in [0, n) whose first tile is <= v
__device__ __forceinline__ int rss_find(const int64_t* __restrict__ plan, int n, int64_t v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plan[(size_t)mid * RSS_INTS + 8] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// what both kernels check of a record before they touch the history or the packet
__device__ __forceinline__ bool rss_record_ok(int64_t slot, int64_t N0, int64_t poff, int64_t n, int slots, int64_t nIn) {
    return slot >= 0 && slot < slots && N0 >= 0 && N0 <= RSS_MAX_COUNT && poff >= 0 && n >= 0 && n <= nIn && poff <= nIn - n;
}

// grid (n_tiles).  LDS: span floats of samples, then the table.
template <bool TAPS_LDS>
__global__ __launch_bounds__(256) void resample_stream_kernel(const float* __restrict__ hist, const float* __restrict__ in,
                                                              float* __restrict__ out, const int64_t* __restrict__ plan,
                                                              const float* __restrict__ table, int half, int K, int p,
                                                              int q, int tile, int span, int n_sess, int slots,
                                                              int64_t nIn, int64_t nOut, int64_t nTiles) {
    extern __shared__ __attribute__((aligned(16))) float rss_lds[];
    const int Kp = (K + 3) & ~3;
    float* xs = rss_lds;
    const float* tab = table;
    if (TAPS_LDS) {
        float* ts = rss_lds + span;                    // span is a multiple of 4: rows stay 16-byte aligned
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
    const int64_t* r = plan + (size_t)rss_find(plan, n_sess, (int64_t)blockIdx.x) * RSS_INTS;
    const int64_t slot = r[0], N0 = r[1], poff = r[2], n = r[3], mfirst = r[4], cnt = r[5], ooff = r[6], t0 = r[8], t1 = r[9];
    // [7] is the commit kernel's: here a closing session differs only in outputs that reach past N1, where the line is zero
    // workgroup-uniform: a record that leaves the extents is skipped
    if (!rss_record_ok(slot, N0, poff, n, slots, nIn) || mfirst < 0 || mfirst > RSS_MAX_OUTPUT || cnt < 0 || cnt > nOut ||
        ooff < 0 || ooff > nOut - cnt || t0 < 0 || t1 > nTiles || t1 - t0 != (cnt + tile - 1) / tile ||
        (int64_t)blockIdx.x < t0 || (int64_t)blockIdx.x >= t1)
        return;
    const int H = K - 1;
    rss_line line;
    line.hist = hist + (size_t)slot * H;
    line.pkt = in + poff;
    line.N0 = N0;
    line.N1 = N0 + n;
    line.H = H;
    const int64_t j0 = ((int64_t)blockIdx.x - t0) * tile;                  // first output of the tile, counted from mfirst
    const int jlast = (int)((j0 + tile < cnt ? j0 + tile : cnt) - 1 - j0);
    const int64_t m0 = mfirst + j0, mlast = m0 + jlast;
    // resample.hip from here on: c0 = m0 q + half = nmax0 p + r0; output m0 + j has c = c0 + j q
    const int64_t c0 = m0 * q + half;
    const int64_t nmax0 = c0 / p;
    const int r0 = (int)(c0 - nmax0 * p);
    const int64_t n_hi = (mlast * q + half) / p;
    const int64_t n_lo = nmax0 - (Kp - 1);
    float* y = out + ooff + j0;

    for (int64_t top = n_hi; top >= n_lo; top -= span) {
        const int64_t w0 = top - span + 1;              // this window holds samples w0 .. top at xs[0 .. span)
        __syncthreads();                                // the table is in place / the last window has been read
        for (int i = threadIdx.x; i < span; i += 256 * RSS_STAGE) {
            float v[RSS_STAGE];
#pragma unroll
            for (int u = 0; u < RSS_STAGE; ++u) v[u] = i + 256 * u < span ? rss_sample(line, w0 + i + 256 * u) : 0.f;
#pragma unroll
            for (int u = 0; u < RSS_STAGE; ++u)
                if (i + 256 * u < span) xs[i + 256 * u] = v[u];
        }
        __syncthreads();
        const int d0 = (int)(nmax0 - w0);
        for (int j = threadIdx.x; j <= jlast; j += 256) {
            const unsigned c = (unsigned)j * (unsigned)q + (unsigned)r0;
            const unsigned dn = c / (unsigned)p;
            const int rr = (int)(c - dn * (unsigned)p);
            const float* row = tab + rr * Kp;
            const int base = d0 + (int)dn;              // xs index of tap 0's sample; tap k reads xs[base - k]
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

// grid (n_sess).  LDS: H floats.
__global__ __launch_bounds__(256) void resample_stream_commit_kernel(float* __restrict__ hist, const float* __restrict__ in,
                                                                     const int64_t* __restrict__ plan, int H, int slots,
                                                                     int64_t nIn) {
    extern __shared__ __attribute__((aligned(16))) float rss_lds[];
    const int64_t* r = plan + (size_t)blockIdx.x * RSS_INTS;
    const int64_t slot = r[0], N0 = r[1], poff = r[2], n = r[3];
    if (!rss_record_ok(slot, N0, poff, n, slots, nIn)) return;
    if (r[7] != 0 || n == 0) return;                    // a closing slot starts afresh; an empty packet moves nothing
    float* h = hist + (size_t)slot * H;
    rss_line line;
    line.hist = h;
    line.pkt = in + poff;
    line.N0 = N0;
    line.N1 = N0 + n;
    line.H = H;
    const int64_t first = line.N1 - H;                  // the new history is x[N1 - H .. N1)
    for (int i = threadIdx.x; i < H; i += 256) rss_lds[i] = rss_sample(line, first + i);
    __syncthreads();
    for (int i = threadIdx.x; i < H; i += 256) h[i] = rss_lds[i];
}

// what the host can see of a ratio: p, q, half = zeros max(p, q), K = ceil((2 half + 1) / p), a history that fits
bool rss_ratio_ok(int half, int K, int p, int q) {
    if (p < 1 || p > RSS_MAX_RATIO || q < 1 || q > RSS_MAX_RATIO) return false;
    const int big = p > q ? p : q;
    if (half < big || half % big != 0 || half / big > RSS_MAX_ZEROS || K != (2 * half + p) / p) return false;
    return K - 1 <= RSS_HIST_MAX;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_resample_stream(const float* hist, const float* in, float* out, const int64_t* plan,
                                      const float* table, int half, int K, int p, int q, int tile, int n_sess, int slots,
                                      int64_t n_in, int64_t n_out, int64_t n_tiles, int taps_in_lds, void* stream) {
    if (!hist || !plan || !table || n_sess < 1 || slots < 1 || taps_in_lds < 0 || taps_in_lds > 1 ||
        !rss_ratio_ok(half, K, p, q))
        return TRUNET_EINVAL;
    if (tile < 256 || tile > RSS_MAX_TILE || tile % 256 != 0) return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (n_in < 0 || n_out < 0 || n_tiles < 0 || n_in > lim || n_out > lim || (n_in > 0 && !in) || (n_out > 0 && !out))
        return TRUNET_EINVAL;
    // sum ceil(outputs / tile) lies in [n_out / tile, n_out / tile + n_sess)
    if (n_tiles * tile < n_out || n_tiles * tile >= n_out + (int64_t)n_sess * tile) return TRUNET_EINVAL;
    const int Kp = (K + 3) & ~3;
    if (taps_in_lds && p * Kp > RSS_TAPS_LDS_MAX) return TRUNET_EINVAL;
    if (n_out == 0) return TRUNET_OK;
    int64_t span = ((int64_t)(tile - 1) * q + p - 1) / p + Kp + 1;
    span = (span + 3) & ~(int64_t)3;
    if (span > RSS_SPAN_MAX) span = RSS_SPAN_MAX;
    const size_t lds = ((size_t)span + (taps_in_lds ? (size_t)p * Kp : 0)) * sizeof(float);
    auto kern = taps_in_lds ? resample_stream_kernel<true> : resample_stream_kernel<false>;
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_tiles), dim3(256), lds, ST, hist, in, out, plan, table, half, K, p, q, tile,
                       (int)span, n_sess, slots, n_in, n_out, n_tiles);
    return trunet_launch_status();
}

extern "C" int trunet_resample_stream_commit(float* hist, const float* in, const int64_t* plan, int half, int K, int p, int q,
                                             int n_sess, int slots, int64_t n_in, void* stream) {
    if (!hist || !plan || n_sess < 1 || slots < 1 || !rss_ratio_ok(half, K, p, q)) return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (n_in < 0 || n_in > lim || (n_in > 0 && !in)) return TRUNET_EINVAL;
    if (n_in == 0) return TRUNET_OK;                    // every packet is empty: no history moves
    const int H = K - 1;
    const size_t lds = (size_t)H * sizeof(float);
    if (hipFuncSetAttribute((const void*)resample_stream_commit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(resample_stream_commit_kernel, dim3((unsigned)n_sess), dim3(256), lds, ST, hist, in, plan, H, slots, n_in);
    return trunet_launch_status();
}
