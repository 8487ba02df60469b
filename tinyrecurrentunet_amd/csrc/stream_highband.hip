// The band above 8 kHz for sessions that arrive in packets (stream_highband.py, StreamPool(highband=)).
// A session's audio x at fs > 16 kHz goes down to lo (16 kHz), through the 16 kHz pool (ys16, whole hops, four hops late)
// and back up (up_y); a second up-resampler plane carries the lo that pairs with ys16 (up_x), and the result is
//   "keep":   out[n] = up_y[n] + (x[n] - up_x[n])
//   "follow": out[n] = fmaf(G[n], x[n] - up_x[n], up_y[n]), the causal gain
//     a[n] = sum_{k = 0 .. 62} hp[k] lo[n - k], b the same on ys16 (zeros left of the session)
//     E_x[j], E_y[j] = sum of a^2, b^2 over hop block j = [128 j, 128 j + 128) n [0, L16)
//     g_c[j] = clamp(sqrt((sum_{i = max(j - 3, 0) .. j} E_y[i] + 1e-10) / (sum_i E_x[i] + 1e-10)), g_min, 1), i ascending
//     s = n pd, D = 128 qd, j = s / D, c = s % D:  G[n] = ((D - c) g_c[max(j - 1, 0)] + c g_c[j]) / D
// Per slot: the x line (samples fed and not yet returned, at most xcap), the lo line (samples of lo whose ys16 has not come
// back, at most 511), and for "follow" the last 62 samples of lo and ys16, the last three block energies and the last two
// block gains.  One int64 plan per call (TRUNET_SHB_INTS per listed session, trunet_hip.h).  The compute kernels only read
// the per-slot state; stream_hb_commit_kernel, after them on the same stream, moves it on (stage in LDS, barrier, write).
// No atomics, nothing read back; every sum has one order whatever the packets were, so neither the cut nor the pool-mates
// change a bit of a session's result.  A record whose extents leave the buffers passed in is skipped, workgroup-uniformly.
#include "common.hpp"
#include "highband_mix.hpp"

namespace {

constexpr int SHB_INTS = TRUNET_SHB_INTS;
constexpr int SHB_TAPS = TRUNET_HB_TAPS;             // 63
constexpr int SHB_HALO = SHB_TAPS - 1;               // 62 samples left of a block
constexpr int SHB_HOP = 128;
constexpr int SHB_LO = TRUNET_SHB_LO_LINE;           // floats of a slot's lo line
constexpr int SHB_XMAX = TRUNET_SHB_MAX_X_LINE;      // floats of a slot's x line, at most
constexpr int SHB_TILE = TRUNET_SHB_TILE;            // samples a workgroup of the pair / join kernels owns: four per thread
constexpr int SHB_MAX_RATIO = 640;
constexpr float SHB_EPS = 1e-10f;
constexpr int64_t SHB_MAX_COUNT = (int64_t)1 << 40;
static_assert(SHB_TILE == 1024 && SHB_LO >= 512 && SHB_XMAX >= SHB_LO, "256 threads, four samples each; one staging buffer");

struct shb_ext {             // what the entry point was given: every record is held against it
    int n_sess, slots, xcap;
    int64_t n_packet, n_up, n_x16, n_paired, n_blocks;
};

struct shb_rec {
    int64_t slot, xc0, xoff, xn, uoff, on, lc0, loff, ln, poff, pn, e0, b0, bn, jt0, closing, pt0, boff;
};

__device__ __forceinline__ bool shb_span_ok(int64_t off, int64_t n, int64_t total) {
    return off >= 0 && n >= 0 && n <= total && off <= total - n;
}

// record i of the plan, and whether it stays inside the extents (uniform over the workgroup that asks)
__device__ __forceinline__ bool shb_load(const int64_t* __restrict__ plan, int i, const shb_ext& e, shb_rec& c) {
    const int64_t* r = plan + (size_t)i * SHB_INTS;
    c = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], r[14], r[15], r[16], r[17]};
    if (c.slot < 0 || c.slot >= e.slots || (c.closing != 0 && c.closing != 1)) return false;
    if (c.xc0 < 0 || c.xc0 > e.xcap || !shb_span_ok(c.xoff, c.xn, e.n_packet) || !shb_span_ok(c.uoff, c.on, e.n_up) ||
        c.on > c.xc0 + c.xn || (!c.closing && c.xc0 + c.xn - c.on > e.xcap))
        return false;
    if (c.lc0 < 0 || c.lc0 > SHB_LO || !shb_span_ok(c.loff, c.ln, e.n_x16) || !shb_span_ok(c.poff, c.pn, e.n_paired) ||
        c.pn > c.lc0 + c.ln || (!c.closing && c.lc0 + c.ln - c.pn > SHB_LO))
        return false;
    if (c.e0 < 0 || c.e0 > SHB_MAX_COUNT || c.b0 < 0 || c.b0 > SHB_MAX_COUNT || !shb_span_ok(c.boff, c.bn, e.n_blocks))
        return false;
    // whole hops before the session ends; only the last block of a closing session may be partial
    return c.closing ? c.bn == (c.pn + SHB_HOP - 1) / SHB_HOP : c.pn == c.bn * SHB_HOP;
}

// the record whose entries [boff + w i, boff' + w (i + 1)) hold entry v: every record owns bn + w entries of a packed array
__device__ __forceinline__ int shb_entry_find(const int64_t* __restrict__ plan, int n, int64_t v, int w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plan[(size_t)mid * SHB_INTS + 17] + (int64_t)w * mid <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// grid (n_pair_tiles): paired[poff + i] = sample i of [lo line | the call's x16], i < pn: the lo whose ys16 came back
__global__ __launch_bounds__(256) void stream_hb_pair_kernel(const float* __restrict__ lo_line, const float* __restrict__ x16,
                                                             float* __restrict__ paired, const int64_t* __restrict__ plan,
                                                             shb_ext e, int64_t n_tiles) {
    const int i = prefix_find(plan + 16, e.n_sess, (int64_t)blockIdx.x, SHB_INTS);
    shb_rec c;
    if (!shb_load(plan, i, e, c)) return;
    const int64_t t = (int64_t)blockIdx.x - c.pt0;
    if (t < 0 || c.pt0 < 0 || c.pt0 > n_tiles || t * SHB_TILE >= c.pn) return;
    const float* line = lo_line + (size_t)c.slot * SHB_LO;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t k = t * SHB_TILE + threadIdx.x + 256 * u;
        if (k < c.pn) paired[c.poff + k] = k < c.lc0 ? line[k] : x16[c.loff + (k - c.lc0)];
    }
}

// grid (n_blocks + 3 n_sess), one wave each.  eline: per record 3 + bn entries (E_x, E_y): the slot's last three blocks,
// then the call's new ones.  A new block is filtered from [the slot's last 62 samples | the call's paired samples], lo and
// ys16 interleaved in LDS, taps ascending, and summed over the wave in wave_sum's fixed order.
__global__ __launch_bounds__(64) void stream_hb_energy_kernel(const float* __restrict__ paired, const float* __restrict__ ys16,
                                                              const f32x2* __restrict__ halo, const f32x2* __restrict__ estate,
                                                              const float* __restrict__ hp, f32x2* __restrict__ eline,
                                                              const int64_t* __restrict__ plan, shb_ext e) {
    __shared__ f32x2 xs[SHB_HOP + SHB_HALO + 2];
    const int64_t v = blockIdx.x;
    const int i = shb_entry_find(plan, e.n_sess, v, 3);
    shb_rec c;
    if (!shb_load(plan, i, e, c)) return;
    const int64_t ent = v - (c.boff + 3 * (int64_t)i);
    if (ent < 0 || ent >= c.bn + 3) return;
    const int lane = threadIdx.x;
    if (ent < 3) {
        if (lane == 0) eline[v] = estate[(size_t)c.slot * 3 + ent];
        return;
    }
    const int64_t b = ent - 3;                           // block b of the call is block b0 + b of the session
    const f32x2* hs = halo + (size_t)c.slot * SHB_HALO;
    const int64_t before = c.b0 * SHB_HOP;               // samples of the session left of the call's first
    for (int k = lane; k < SHB_HOP + SHB_HALO + 2; k += 64) {
        const int64_t pos = b * SHB_HOP + k;             // position in [halo | paired]
        f32x2 val = {0.f, 0.f};
        if (pos < SHB_HALO) {
            if (before + pos - SHB_HALO >= 0) val = hs[pos];
        } else if (pos - SHB_HALO < c.pn) {
            val = f32x2{paired[c.poff + pos - SHB_HALO], ys16[c.poff + pos - SHB_HALO]};
        }
        xs[k] = val;
    }
    __syncthreads();
    // samples s = 2 lane and s + 1 of the block; tap k of sample s reads xs[s + 62 - k], and sample s + 1 read the same
    // value one tap earlier
    const int s = 2 * lane;
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    f32x2 cur = xs[s + SHB_HALO + 1];
#pragma unroll
    for (int k = 0; k < SHB_TAPS; ++k) {
        const f32x2 nxt = xs[s + SHB_HALO - k];
        const float h = hp[k];
        a1 = fmaf(h, cur.x, a1);
        b1 = fmaf(h, cur.y, b1);
        a0 = fmaf(h, nxt.x, a0);
        b0 = fmaf(h, nxt.y, b0);
        cur = nxt;
    }
    const int64_t left = c.pn - b * SHB_HOP;             // samples of the block that exist: 128, fewer in a closing session's last
    if (s >= left) a0 = b0 = 0.f;
    if (s + 1 >= left) a1 = b1 = 0.f;
    const float ex = wave_sum(fmaf(a1, a1, a0 * a0));
    const float ey = wave_sum(fmaf(b1, b1, b0 * b0));
    if (lane == 0) eline[v] = f32x2{ex, ey};
}

// grid (ceil((n_blocks + 2 n_sess) / 256)), a thread per entry of gline: per record the slot's last two block gains, then
// the gains of the call's new blocks, each from the four trailing block energies added in ascending order
__global__ __launch_bounds__(256) void stream_hb_gain_kernel(const f32x2* __restrict__ eline, const float* __restrict__ gstate,
                                                             float* __restrict__ gline, const int64_t* __restrict__ plan,
                                                             shb_ext e, float g_min) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= e.n_blocks + 2 * (int64_t)e.n_sess) return;
    const int i = shb_entry_find(plan, e.n_sess, v, 2);
    shb_rec c;
    if (!shb_load(plan, i, e, c)) return;
    const int64_t ent = v - (c.boff + 2 * (int64_t)i);
    if (ent < 0 || ent >= c.bn + 2) return;
    if (ent < 2) {
        gline[v] = gstate[(size_t)c.slot * 2 + ent];
        return;
    }
    const int64_t b = ent - 2, j = c.b0 + b;
    const f32x2* el = eline + c.boff + 3 * (int64_t)i + 3 + b;           // the block's own energy; older ones lie before it
    float ex = 0.f, ey = 0.f;
#pragma unroll
    for (int d = 3; d >= 0; --d) {
        if (j - d < 0) continue;
        const f32x2 en = el[-d];
        ex += en.x;
        ey += en.y;
    }
    const float r = sqrtf((ey + SHB_EPS) / (ex + SHB_EPS));
    gline[v] = fminf(fmaxf(r, g_min), 1.f);
}

// grid (n_join_tiles): a workgroup owns SHB_TILE outputs of one session, counted from its first output of the call.
// x comes from [x line | packet]; up_y, up_x and out are packed alike (uoff).
template <bool FOLLOW>
__global__ __launch_bounds__(256) void stream_hb_join_kernel(const float* __restrict__ up_y, const float* __restrict__ up_x,
                                                             const float* __restrict__ x_line, const float* __restrict__ packet,
                                                             const float* __restrict__ gline, float* __restrict__ out,
                                                             const int64_t* __restrict__ plan, shb_ext e, int64_t n_tiles,
                                                             int pd, int qd) {
    const int i = prefix_find(plan + 14, e.n_sess, (int64_t)blockIdx.x, SHB_INTS);
    shb_rec c;
    if (!shb_load(plan, i, e, c)) return;
    const int64_t t = (int64_t)blockIdx.x - c.jt0;
    if (t < 0 || c.jt0 < 0 || c.jt0 > n_tiles || t * SHB_TILE >= c.on) return;
    const int64_t n0 = t * SHB_TILE;
    const int cnt = (int)(c.on - n0 < SHB_TILE ? c.on - n0 : SHB_TILE);
    const float* xl = x_line + (size_t)c.slot * e.xcap;
    const float* py = up_y + c.uoff + n0;
    const float* pu = up_x + c.uoff + n0;
    float* po = out + c.uoff + n0;
    const unsigned D = (unsigned)SHB_HOP * (unsigned)qd;
    int64_t tt = 0;
    unsigned ct = 0;
    const float* gl = gline;
    if (FOLLOW) {
        const int64_t s = (c.e0 + n0) * pd;              // below 2^51
        tt = s / D;
        ct = (unsigned)(s - tt * D);
        gl = gline + c.boff + 2 * (int64_t)i;            // entry k: g_c[b0 - 2 + k]
    }
    const int64_t last = c.bn + 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = threadIdx.x + 256 * u;
        if (k >= cnt) break;
        const int64_t n = n0 + k;
        const float xv = n < c.xc0 ? xl[n] : packet[c.xoff + (n - c.xc0)];
        float G = 1.f;
        if (FOLLOW) {
            unsigned cc = ct + (unsigned)k * (unsigned)pd;               // below 128 * 640 + 1024 * 640
            const unsigned dt = cc / D;
            cc -= dt * D;
            const int64_t j = tt + dt;
            // the plan keeps both inside [b0 - 2, b0 + bn) (causality, section 3r); the clamp keeps a record that does not
            // inside its own entries
            int64_t ka = (j > 0 ? j - 1 : 0) - c.b0 + 2, kb = j - c.b0 + 2;
            ka = ka < 0 ? 0 : (ka > last ? last : ka);
            kb = kb < 0 ? 0 : (kb > last ? last : kb);
            G = hb_lerp(gl[ka], gl[kb], cc, D);
        }
        po[k] = hb_mix<FOLLOW>(py[k], pu[k], xv, G);
    }
}

// grid (n_sess), after the compute kernels on the same stream.  x line <- [x line | packet] without its first `on` samples;
// lo line <- [lo line | x16] without its first pn; "follow": the last 62 of [halo | paired], the last three of eline and the
// last two of gline.  A closing slot starts afresh: nothing of it is kept.
__global__ __launch_bounds__(256) void stream_hb_commit_kernel(float* __restrict__ x_line, const float* __restrict__ packet,
                                                               float* __restrict__ lo_line, const float* __restrict__ x16,
                                                               f32x2* __restrict__ halo, const float* __restrict__ paired,
                                                               const float* __restrict__ ys16, f32x2* __restrict__ estate,
                                                               const f32x2* __restrict__ eline, float* __restrict__ gstate,
                                                               const float* __restrict__ gline,
                                                               const int64_t* __restrict__ plan, shb_ext e, int follow) {
    __shared__ float stage[SHB_XMAX];
    shb_rec c;
    if (!shb_load(plan, (int)blockIdx.x, e, c) || c.closing) return;
    if (c.on > 0 || c.xn > 0) {
        float* xl = x_line + (size_t)c.slot * e.xcap;
        const int keep = (int)(c.xc0 + c.xn - c.on);
        for (int k = threadIdx.x; k < keep; k += 256) {
            const int64_t n = c.on + k;
            stage[k] = n < c.xc0 ? xl[n] : packet[c.xoff + (n - c.xc0)];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < keep; k += 256) xl[k] = stage[k];
        __syncthreads();
    }
    if (c.pn > 0 || c.ln > 0) {
        float* ll = lo_line + (size_t)c.slot * SHB_LO;
        const int keep = (int)(c.lc0 + c.ln - c.pn);
        for (int k = threadIdx.x; k < keep; k += 256) {
            const int64_t n = c.pn + k;
            stage[k] = n < c.lc0 ? ll[n] : x16[c.loff + (n - c.lc0)];
        }
        __syncthreads();
        for (int k = threadIdx.x; k < keep; k += 256) ll[k] = stage[k];
        __syncthreads();
    }
    if (!follow || c.pn == 0) return;                    // no new ys16: halo, energies and gains stay
    f32x2* hs = halo + (size_t)c.slot * SHB_HALO;
    f32x2* st2 = reinterpret_cast<f32x2*>(stage);
    if (threadIdx.x < SHB_HALO) {
        const int64_t pos = c.pn + threadIdx.x;          // position in [halo | paired]
        st2[threadIdx.x] = pos < SHB_HALO ? hs[pos]
                                          : f32x2{paired[c.poff + pos - SHB_HALO], ys16[c.poff + pos - SHB_HALO]};
    }
    __syncthreads();
    if (threadIdx.x < SHB_HALO) hs[threadIdx.x] = st2[threadIdx.x];
    // eline and gline are the call's own arrays, not the state: no staging needed
    if (threadIdx.x < 3) estate[(size_t)c.slot * 3 + threadIdx.x] = eline[c.boff + 3 * (int64_t)blockIdx.x + c.bn + threadIdx.x];
    if (threadIdx.x < 2) gstate[(size_t)c.slot * 2 + threadIdx.x] = gline[c.boff + 2 * (int64_t)blockIdx.x + c.bn + threadIdx.x];
}

const int64_t SHB_LIM = ((int64_t)1 << 31) - 1;

bool shb_total_ok(int64_t n, const void* p) { return n >= 0 && n <= SHB_LIM && (n == 0 || p); }

// what the host can see of the extents; the tiles of a packed array of n samples over n_sess sessions
bool shb_ext_ok(const shb_ext& e) {
    return e.n_sess >= 1 && e.slots >= 1 && e.xcap >= 1 && e.xcap <= SHB_XMAX && e.n_packet >= 0 && e.n_packet <= SHB_LIM &&
           e.n_up >= 0 && e.n_up <= SHB_LIM && e.n_x16 >= 0 && e.n_x16 <= SHB_LIM && e.n_paired >= 0 &&
           e.n_paired <= SHB_LIM && e.n_blocks >= 0 && e.n_blocks * SHB_HOP >= e.n_paired &&
           e.n_blocks * SHB_HOP < e.n_paired + (int64_t)e.n_sess * SHB_HOP;
}

bool shb_tiles_ok(int64_t n_tiles, int64_t n, int n_sess) {
    return n_tiles >= 0 && n_tiles * SHB_TILE < n + (int64_t)n_sess * SHB_TILE;
}

}  // namespace

extern "C" int trunet_stream_highband_pair(const float* lo_line, const float* x16, float* paired, const int64_t* plan,
                                           int n_sess, int slots, int xcap, int64_t n_packet, int64_t n_up, int64_t n_x16,
                                           int64_t n_paired, int64_t n_blocks, int64_t n_tiles, void* stream) {
    const shb_ext e = {n_sess, slots, xcap, n_packet, n_up, n_x16, n_paired, n_blocks};
    if (!lo_line || !plan || !shb_ext_ok(e) || !shb_total_ok(n_x16, x16) || !shb_total_ok(n_paired, paired) ||
        !shb_tiles_ok(n_tiles, n_paired, n_sess))
        return TRUNET_EINVAL;
    if (n_tiles == 0) return TRUNET_OK;
    hipLaunchKernelGGL(stream_hb_pair_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, lo_line, x16, paired,
                       plan, e, n_tiles);
    return trunet_launch_status();
}

extern "C" int trunet_stream_highband_gains(const float* paired, const float* ys16, const float* halo, const float* estate,
                                            const float* gstate, const float* hp, float* eline, float* gline,
                                            const int64_t* plan, int n_sess, int slots, int xcap, int64_t n_packet,
                                            int64_t n_up, int64_t n_x16, int64_t n_paired, int64_t n_blocks, float g_min,
                                            void* stream) {
    const shb_ext e = {n_sess, slots, xcap, n_packet, n_up, n_x16, n_paired, n_blocks};
    if (!halo || !estate || !gstate || !hp || !eline || !gline || !plan || !shb_ext_ok(e) || !shb_total_ok(n_paired, paired) ||
        !shb_total_ok(n_paired, ys16) || !(g_min > 0.f) || !(g_min <= 1.f))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_hb_energy_kernel, dim3((unsigned)(n_blocks + 3 * (int64_t)n_sess)), dim3(64), 0,
                       (hipStream_t)stream, paired, ys16, reinterpret_cast<const f32x2*>(halo),
                       reinterpret_cast<const f32x2*>(estate), hp, reinterpret_cast<f32x2*>(eline), plan, e);
    if (trunet_launch_status() != TRUNET_OK) return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(stream_hb_gain_kernel, dim3((unsigned)((n_blocks + 2 * (int64_t)n_sess + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const f32x2*>(eline), gstate, gline, plan, e, g_min);
    return trunet_launch_status();
}

extern "C" int trunet_stream_highband_join(const float* up_y, const float* up_x, const float* x_line, const float* packet,
                                           const float* gline, float* out, const int64_t* plan, int n_sess, int slots,
                                           int xcap, int64_t n_packet, int64_t n_up, int64_t n_x16, int64_t n_paired,
                                           int64_t n_blocks, int64_t n_tiles, int pd, int qd, int mode, void* stream) {
    const shb_ext e = {n_sess, slots, xcap, n_packet, n_up, n_x16, n_paired, n_blocks};
    if (!x_line || !plan || !shb_ext_ok(e) || !shb_total_ok(n_up, up_y) || !shb_total_ok(n_up, up_x) ||
        !shb_total_ok(n_up, out) || !shb_total_ok(n_packet, packet) || !shb_tiles_ok(n_tiles, n_up, n_sess) || pd < 1 ||
        qd <= pd || qd > SHB_MAX_RATIO || (mode != TRUNET_HB_KEEP && mode != TRUNET_HB_FOLLOW) ||
        (mode == TRUNET_HB_FOLLOW && !gline))
        return TRUNET_EINVAL;
    if (n_tiles == 0) return TRUNET_OK;
    if (mode == TRUNET_HB_FOLLOW)
        hipLaunchKernelGGL(stream_hb_join_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, up_y, up_x,
                           x_line, packet, gline, out, plan, e, n_tiles, pd, qd);
    else
        hipLaunchKernelGGL(stream_hb_join_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, up_y, up_x,
                           x_line, packet, gline, out, plan, e, n_tiles, pd, qd);
    return trunet_launch_status();
}

extern "C" int trunet_stream_highband_commit(float* x_line, const float* packet, float* lo_line, const float* x16, float* halo,
                                             const float* paired, const float* ys16, float* estate, const float* eline,
                                             float* gstate, const float* gline, const int64_t* plan, int n_sess, int slots,
                                             int xcap, int64_t n_packet, int64_t n_up, int64_t n_x16, int64_t n_paired,
                                             int64_t n_blocks, int mode, void* stream) {
    const shb_ext e = {n_sess, slots, xcap, n_packet, n_up, n_x16, n_paired, n_blocks};
    const bool follow = mode == TRUNET_HB_FOLLOW;
    if (!x_line || !lo_line || !plan || !shb_ext_ok(e) || !shb_total_ok(n_packet, packet) || !shb_total_ok(n_x16, x16) ||
        !shb_total_ok(n_paired, paired) || (mode != TRUNET_HB_KEEP && !follow) ||
        (follow && (!halo || !estate || !gstate || !eline || !gline || !shb_total_ok(n_paired, ys16))))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(stream_hb_commit_kernel, dim3((unsigned)n_sess), dim3(256), 0, (hipStream_t)stream, x_line, packet,
                       lo_line, x16, reinterpret_cast<f32x2*>(halo), paired, ys16, reinterpret_cast<f32x2*>(estate),
                       reinterpret_cast<const f32x2*>(eline), gstate, gline, plan, e, follow ? 1 : 0);
    return trunet_launch_status();
}
