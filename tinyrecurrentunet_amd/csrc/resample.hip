// Rational resampling (resample.py), of whole utterances and of streaming sessions (3m):
//   y[m] = p sum_n h[m q - n p + half] x[n],  m < ceil(L p / q),  h = 2 half + 1 taps, zero outside
// (scipy.signal.resample_poly(x, p, q, window=h)).  Unlike metrics.hip's resample_poly_kernel (STOI's 10 kHz resampler,
// one global load per tap) a workgroup owns one tile of `tile` consecutive outputs of ONE signal and stages the tile's
// input span in LDS once: zeros outside the signal, so the tap loop has no bounds test and no global load of a sample.
// The taps come phase-major, table[r][k] = h[r + k p] in rows of Kp = round_up(K, 4) floats (zero padded): the K taps of
// output m (r = (m q + half) % p, n = (m q + half) / p - k) are one contiguous row, read four at a time from LDS
// (TAPS_LDS) or from L2.  Every output accumulates in fp32 with k ascending, then (float)p * acc.  A span longer than
// RS_SPAN_MAX floats (only ratios far below 1: q / p above 16 or so) is staged in windows of RS_SPAN_MAX, highest
// samples first, which keeps k ascending.
// All of that is rs_tile, once; the two kernels differ in where a tile's samples come from (its Src argument):
// resample_rational_kernel: B utterances of any lengths, packed back to back; tiles are counted from an utterance's first
//   output and do not depend on the batch, so an utterance's result is bit for bit independent of its batch-mates.
// resample_stream_kernel: a session that had N0 samples before the call and brings a packet of n is the LINE
//     hist[slot] (x[N0 - H, N0), H = K - 1)  ++  in[poff, poff + n)
//   with zeros left of sample 0 and right of N1 = N0 + n (only a closing session's outputs reach there); tiles are
//   counted from the session's first output of the call.  The next output of a session reads no sample below N0 - H: it
//   is m = ceil((N0 p - half) / q) or later, so m q + half >= N0 p, nmax >= N0 and nmax - (K - 1) >= N0 - H.  So however
//   a session is cut into packets its outputs are bit for bit those of resample_rational_kernel on the whole.
// plan: (n_sess, TRUNET_RS_STREAM_INTS) int64, one record per listed session:
//   [0] slot  [1] N0  [2] poff  [3] n  [4] first output m0  [5] outputs  [6] offset in `out`  [7] closing  [8], [9] the
//   session's tiles [t0, t1) of the grid, t1 - t0 = ceil(outputs / tile).
// resample_stream_kernel reads hist only.  resample_stream_commit_kernel, after it on the same stream: one workgroup per
// session, hist[slot] <- the last H samples of the line, through LDS (every read of the old history comes before the first
// write).  A record whose slot, packet extent, output extent or tiles lie outside the extents passed in is skipped,
// workgroup-uniformly.
#include "common.hpp"

namespace {

constexpr int RS_MAX_RATIO = 640;
constexpr int RS_MAX_ZEROS = 32;                 // half <= 32 max(p, q)
constexpr int RS_MAX_TILE = TRUNET_RS_MAX_TILE;
constexpr int RS_SPAN_MAX = TRUNET_RS_SPAN_MAX;  // floats of input staged per window (18 KiB)
constexpr int RS_STAGE = 6;                      // loads a thread keeps in flight while it stages
constexpr int RS_TAPS_LDS_MAX = TRUNET_RS_TAPS_LDS_MAX;  // floats of the tap table that may live in LDS (64 KiB)
constexpr int RS_INTS = TRUNET_RS_STREAM_INTS;
constexpr int64_t RS_MAX_COUNT = (int64_t)1 << 40;       // samples of a session (resample.py: MAX_SESSION)
constexpr int64_t RS_MAX_OUTPUT = (int64_t)1 << 50;      // its outputs, at most 640 times as many: m q + half stays inside int64

// sample sources: sample n of the signal, zero outside it
struct rs_signal {
    const float* x;          // an utterance of len samples
    int64_t len;
    __device__ __forceinline__ float operator()(int64_t n) const { return n >= 0 && n < len ? x[n] : 0.f; }
};

struct rss_line {
    const float* hist;       // the slot's H history samples, x[N0 - H .. N0)
    const float* pkt;        // the packet, x[N0 .. N1)
    int64_t N0, N1;
    int H;
    // zero outside [0, N1) and below what the history keeps
    __device__ __forceinline__ float operator()(int64_t n) const {
        if (n < 0 || n >= N1) return 0.f;
        if (n >= N0) return pkt[n - N0];
        const int64_t back = N0 - n;             // 1: the newest history sample
        return back <= H ? hist[H - back] : 0.f;
    }
};

// the p x Kp tap table -> LDS at ts (16-byte aligned), which it returns; the first barrier of rs_tile makes it visible
__device__ __forceinline__ const float* rs_stage_table(const float* __restrict__ table, float* ts, int p, int Kp) {
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
    return ts;
}

// outputs m0 .. m0 + jlast of the signal `x` -> y[0 .. jlast]; xs: span floats of LDS, tab: the table (LDS or global)
template <class Src>
__device__ __forceinline__ void rs_tile(const Src& x, const float* tab, float* xs, float* __restrict__ y, int64_t m0,
                                        int jlast, int half, int K, int Kp, int p, int q, int span) {
    // samples the tile reads: n_lo .. n_hi, n_hi the first sample of its last output, n_lo the last of its first.
    // c0 = m0 q + half = nmax0 p + r0; output m0 + j then has c = c0 + j q, so 32-bit arithmetic does per output
    const int64_t c0 = m0 * q + half;
    const int64_t nmax0 = c0 / p;
    const int r0 = (int)(c0 - nmax0 * p);
    const int64_t n_hi = ((m0 + jlast) * q + half) / p;
    const int64_t n_lo = nmax0 - (Kp - 1);

    for (int64_t top = n_hi; top >= n_lo; top -= span) {
        const int64_t w0 = top - span + 1;              // this window holds samples w0 .. top at xs[0 .. span)
        __syncthreads();                                // the table is in place / the last window has been read
        for (int i = threadIdx.x; i < span; i += 256 * RS_STAGE) {      // RS_STAGE loads in flight per thread
            float v[RS_STAGE];
#pragma unroll
            for (int u = 0; u < RS_STAGE; ++u) v[u] = i + 256 * u < span ? x(w0 + i + 256 * u) : 0.f;
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
    // span is a multiple of 4: the table's rows stay 16-byte aligned behind the samples
    const float* tab = TAPS_LDS ? rs_stage_table(table, rs_lds + span, p, Kp) : table;
    const int b = prefix_find(to, B, (int64_t)blockIdx.x);
    const int64_t i0 = io[b], i1 = io[b + 1], o0 = oo[b], o1 = oo[b + 1], t0 = to[b], t1 = to[b + 1];
    // workgroup-uniform: an utterance whose offsets contradict each other is skipped
    if (i0 < 0 || i1 > nIn || i1 < i0 || o0 < 0 || o1 > nOut || o1 - o0 != ((i1 - i0) * p + q - 1) / q || t0 < 0 ||
        t1 > nTiles || t1 - t0 != (o1 - o0 + tile - 1) / tile || (int64_t)blockIdx.x < t0 || (int64_t)blockIdx.x >= t1)
        return;
    const int64_t M = o1 - o0;
    const int64_t m0 = ((int64_t)blockIdx.x - t0) * tile;
    const int jlast = (int)((m0 + tile < M ? m0 + tile : M) - 1 - m0);
    const rs_signal x = {in + (size_t)blockIdx.y * nIn + i0, i1 - i0};
    rs_tile(x, tab, rs_lds, out + (size_t)blockIdx.y * nOut + o0 + m0, m0, jlast, half, K, Kp, p, q, span);
}

// what both stream kernels check of a record before they touch the history or the packet
__device__ __forceinline__ bool rss_record_ok(int64_t slot, int64_t N0, int64_t poff, int64_t n, int slots, int64_t nIn) {
    return slot >= 0 && slot < slots && N0 >= 0 && N0 <= RS_MAX_COUNT && poff >= 0 && n >= 0 && n <= nIn && poff <= nIn - n;
}

// grid (n_tiles).  LDS: span floats of samples, then the table.
template <bool TAPS_LDS>
__global__ __launch_bounds__(256) void resample_stream_kernel(const float* __restrict__ hist, const float* __restrict__ in,
                                                              float* __restrict__ out, const int64_t* __restrict__ plan,
                                                              const float* __restrict__ table, int half, int K, int p,
                                                              int q, int tile, int span, int n_sess, int slots,
                                                              int64_t nIn, int64_t nOut, int64_t nTiles) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int Kp = (K + 3) & ~3;
    // span is a multiple of 4: the table's rows stay 16-byte aligned behind the samples
    const float* tab = TAPS_LDS ? rs_stage_table(table, rs_lds + span, p, Kp) : table;
    // the session whose first tile [8] is the largest <= this one
    const int64_t* r = plan + (size_t)prefix_find(plan + 8, n_sess, (int64_t)blockIdx.x, RS_INTS) * RS_INTS;
    const int64_t slot = r[0], N0 = r[1], poff = r[2], n = r[3], mfirst = r[4], cnt = r[5], ooff = r[6], t0 = r[8], t1 = r[9];
    // [7] is the commit kernel's: here a closing session differs only in outputs that reach past N1, where the line is zero
    // workgroup-uniform: a record that leaves the extents is skipped
    if (!rss_record_ok(slot, N0, poff, n, slots, nIn) || mfirst < 0 || mfirst > RS_MAX_OUTPUT || cnt < 0 || cnt > nOut ||
        ooff < 0 || ooff > nOut - cnt || t0 < 0 || t1 > nTiles || t1 - t0 != (cnt + tile - 1) / tile ||
        (int64_t)blockIdx.x < t0 || (int64_t)blockIdx.x >= t1)
        return;
    const int64_t j0 = ((int64_t)blockIdx.x - t0) * tile;                  // first output of the tile, counted from mfirst
    const int jlast = (int)((j0 + tile < cnt ? j0 + tile : cnt) - 1 - j0);
    const rss_line x = {hist + (size_t)slot * (K - 1), in + poff, N0, N0 + n, K - 1};
    rs_tile(x, tab, rs_lds, out + ooff + j0, mfirst + j0, jlast, half, K, Kp, p, q, span);
}

// grid (n_sess).  LDS: H floats.
__global__ __launch_bounds__(256) void resample_stream_commit_kernel(float* __restrict__ hist, const float* __restrict__ in,
                                                                     const int64_t* __restrict__ plan, int H, int slots,
                                                                     int64_t nIn) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    const int64_t* r = plan + (size_t)blockIdx.x * RS_INTS;
    const int64_t slot = r[0], N0 = r[1], poff = r[2], n = r[3];
    if (!rss_record_ok(slot, N0, poff, n, slots, nIn)) return;
    if (r[7] != 0 || n == 0) return;                    // a closing slot starts afresh; an empty packet moves nothing
    float* h = hist + (size_t)slot * H;
    const rss_line line = {h, in + poff, N0, N0 + n, H};
    const int64_t first = line.N1 - H;                  // the new history is x[N1 - H .. N1)
    for (int i = threadIdx.x; i < H; i += 256) rs_lds[i] = line(first + i);
    __syncthreads();
    for (int i = threadIdx.x; i < H; i += 256) h[i] = rs_lds[i];
}

// what the host can see of a ratio: p, q, half = zeros max(p, q), K = ceil((2 half + 1) / p)
bool rs_ratio_ok(int half, int K, int p, int q) {
    if (p < 1 || p > RS_MAX_RATIO || q < 1 || q > RS_MAX_RATIO) return false;
    const int big = p > q ? p : q;
    return half >= big && half % big == 0 && half / big <= RS_MAX_ZEROS && K == (2 * half + p) / p;
}

bool rs_tile_ok(int tile) { return tile >= 256 && tile <= RS_MAX_TILE && tile % 256 == 0; }

// floats staged per window: the whole span of a full tile if it fits, else windows of RS_SPAN_MAX
int rs_span(int tile, int p, int q, int Kp) {
    const int64_t span = (((int64_t)(tile - 1) * q + p - 1) / p + Kp + 1 + 3) & ~(int64_t)3;
    return span > RS_SPAN_MAX ? RS_SPAN_MAX : (int)span;
}

size_t rs_lds_bytes(int span, int p, int Kp, int taps_in_lds) {
    return ((size_t)span + (taps_in_lds ? (size_t)p * Kp : 0)) * sizeof(float);
}

template <class... P, class... A>
int rs_launch(void (*kern)(P...), dim3 grid, size_t lds, void* stream, A... args) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, (hipStream_t)stream, args...);
    return trunet_launch_status();
}

}  // namespace

extern "C" int trunet_resample_rational(const float* in, float* out, const int64_t* in_off, const int64_t* out_off,
                                        const int64_t* tile_off, const float* table, int half, int K, int p, int q,
                                        int tile, int B, int64_t total_in, int64_t total_out, int64_t total_tiles,
                                        int nsig, int taps_in_lds, void* stream) {
    if (!in || !out || !in_off || !out_off || !tile_off || !table || B < 1 || nsig < 1 || nsig > 2 || taps_in_lds < 0 ||
        taps_in_lds > 1 || !rs_ratio_ok(half, K, p, q) || !rs_tile_ok(tile))
        return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (total_in < 0 || total_out < 0 || total_tiles < 0 || total_in > lim || total_out > lim) return TRUNET_EINVAL;
    // sum ceil(L_b p / q) lies in [total_in p / q, total_in p / q + B), sum ceil(M_b / tile) likewise
    if (total_out * q < total_in * p || total_out * q >= total_in * p + (int64_t)B * q) return TRUNET_EINVAL;
    if (total_tiles * tile < total_out || total_tiles * tile >= total_out + (int64_t)B * tile) return TRUNET_EINVAL;
    const int Kp = (K + 3) & ~3;
    if (taps_in_lds && p * Kp > RS_TAPS_LDS_MAX) return TRUNET_EINVAL;
    if (total_out == 0) return TRUNET_OK;
    const int span = rs_span(tile, p, q, Kp);
    return rs_launch(taps_in_lds ? resample_rational_kernel<true> : resample_rational_kernel<false>,
                     dim3((unsigned)total_tiles, nsig), rs_lds_bytes(span, p, Kp, taps_in_lds), stream, in, out, in_off,
                     out_off, tile_off, table, half, K, p, q, tile, span, B, total_in, total_out, total_tiles);
}

extern "C" int trunet_resample_stream(const float* hist, const float* in, float* out, const int64_t* plan,
                                      const float* table, int half, int K, int p, int q, int tile, int n_sess, int slots,
                                      int64_t n_in, int64_t n_out, int64_t n_tiles, int taps_in_lds, void* stream) {
    if (!hist || !plan || !table || n_sess < 1 || slots < 1 || taps_in_lds < 0 || taps_in_lds > 1 ||
        !rs_ratio_ok(half, K, p, q) || K - 1 > TRUNET_RS_STREAM_MAX_HISTORY || !rs_tile_ok(tile))
        return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (n_in < 0 || n_out < 0 || n_tiles < 0 || n_in > lim || n_out > lim || (n_in > 0 && !in) || (n_out > 0 && !out))
        return TRUNET_EINVAL;
    // sum ceil(outputs / tile) lies in [n_out / tile, n_out / tile + n_sess)
    if (n_tiles * tile < n_out || n_tiles * tile >= n_out + (int64_t)n_sess * tile) return TRUNET_EINVAL;
    const int Kp = (K + 3) & ~3;
    if (taps_in_lds && p * Kp > RS_TAPS_LDS_MAX) return TRUNET_EINVAL;
    if (n_out == 0) return TRUNET_OK;
    const int span = rs_span(tile, p, q, Kp);
    return rs_launch(taps_in_lds ? resample_stream_kernel<true> : resample_stream_kernel<false>, dim3((unsigned)n_tiles),
                     rs_lds_bytes(span, p, Kp, taps_in_lds), stream, hist, in, out, plan, table, half, K, p, q, tile, span,
                     n_sess, slots, n_in, n_out, n_tiles);
}

extern "C" int trunet_resample_stream_commit(float* hist, const float* in, const int64_t* plan, int half, int K, int p, int q,
                                             int n_sess, int slots, int64_t n_in, void* stream) {
    if (!hist || !plan || n_sess < 1 || slots < 1 || !rs_ratio_ok(half, K, p, q) || K - 1 > TRUNET_RS_STREAM_MAX_HISTORY)
        return TRUNET_EINVAL;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (n_in < 0 || n_in > lim || (n_in > 0 && !in)) return TRUNET_EINVAL;
    if (n_in == 0) return TRUNET_OK;                    // every packet is empty: no history moves
    return rs_launch(resample_stream_commit_kernel, dim3((unsigned)n_sess), (size_t)(K - 1) * sizeof(float), stream, hist, in,
                     plan, K - 1, slots, n_in);
}
