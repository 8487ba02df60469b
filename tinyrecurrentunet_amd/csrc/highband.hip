// The band above 8 kHz around a 16 kHz enhancement (highband.py).  Audio x at fs > 16 kHz was resampled
// to lo (16 kHz), enhanced to y16, and both went back up: up_y = U(y16), up_x = U(lo).  hb = x - up_x is what the
// resampler's low-pass removed; the result is up_y + G hb with G = 1 ("keep") or the net's own suppression just below the
// band edge ("follow"):
//   a = hp * lo, b = hp * y16                   63-tap zero-phase high-pass (4 kHz at 16 kHz), "same", zeros outside [0, L16)
//   E_x[j], E_y[j] = sum of a^2, b^2 over hop block j = [128 j, 128 j + 128) n [0, L16)
//   e[t] = E[t - 2] + E[t - 1] + E[t] + E[t + 1] (the blocks that exist),  t < T = 1 + L16 / 128
//   g[t] = clamp(sqrt((e_y[t] + 1e-10) / (e_x[t] + 1e-10)), g_min, 1)
//   G[n] = (1 - al) g[t0] + al g[min(t0 + 1, T - 1)],  s = n pd,  t0 = s / (128 qd),  al = (s % (128 qd)) / (128 qd)
// highband_energy_kernel: a workgroup owns HB_RUN hop blocks of ONE utterance, counted from the utterance's first sample,
//   stages their samples with the 31-sample halo in LDS (lo and y16 interleaved, zeros outside the utterance), filters with
//   k ascending and sums each block over one wave in the fixed order of wave_sum -> (E_x, E_y) per block.
// highband_gain_kernel: a thread per frame, the four block energies added with j ascending, the clamp.
// highband_join_kernel: a workgroup owns HJ_TILE consecutive samples of one utterance; one 64-bit division per workgroup,
//   32-bit arithmetic per sample; float4 accesses where the utterance's offsets are aligned, scalar ones otherwise, the
//   same expression either way.
// No workgroup reads another's results within a launch, there are no atomics, and an utterance's results are bit for bit
// independent of its batch-mates.  Workgroups find their utterance without a tile table: utterance b, whose prefix offset
// is off[b], owns the grid slots [off[b] / W + b, off[b + 1] / W + b + 1), at least ceil((off[b + 1] - off[b]) / W) of
// them; a slot past the utterance's last tile returns.
#include "common.hpp"
#include "highband_mix.hpp"

namespace {

constexpr int HB_HALF = (TRUNET_HB_TAPS - 1) / 2;   // 31
constexpr int HB_HOP = 128;
constexpr int HB_RUN = TRUNET_HB_RUN;                // hop blocks per workgroup: four per wave
constexpr int HB_SPAN = HB_RUN * HB_HOP + 2 * HB_HALF;
constexpr int HJ_TILE = TRUNET_HB_JOIN_TILE;         // samples per workgroup of the join: four float4 per thread
static_assert(HB_RUN % 4 == 0 && HJ_TILE % 1024 == 0, "four waves share a run; a thread of the join moves float4s");
constexpr int HB_MAX_RATIO = 640;
constexpr float HB_EPS = 1e-10f;

// largest b in [0, n) with off[b] / w + b <= v: the utterance that owns grid slot v (see the head of the file).  Any b in
// [0, n) for a corrupt table: the caller validates what it gets.
__device__ __forceinline__ int slot_find(const int64_t* __restrict__ off, int n, int64_t v, int w) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] / w + mid <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// T_b = 1 + L_b / 128 of an utterance of L samples at 16 kHz, inside the declared totals
__device__ __forceinline__ bool frames_ok(int64_t f0, int64_t f1, int64_t L16, int64_t nT) {
    return f0 >= 0 && f1 <= nT && f1 - f0 == 1 + L16 / HB_HOP;
}

// grid (total_frames / HB_RUN + B).  energy: (total_frames, 2), block j of utterance b at frame_off[b] + j.
__global__ __launch_bounds__(256) void highband_energy_kernel(const float* __restrict__ lo, const float* __restrict__ y16,
                                                              const int64_t* __restrict__ so, const int64_t* __restrict__ fo,
                                                              const float* __restrict__ hp, f32x2* __restrict__ energy, int B,
                                                              int64_t nS, int64_t nT) {
    __shared__ __attribute__((aligned(16))) f32x2 xs[HB_SPAN];
    const int b = slot_find(fo, B, (int64_t)blockIdx.x, HB_RUN);
    const int64_t i0 = so[b], i1 = so[b + 1], f0 = fo[b], f1 = fo[b + 1];
    // workgroup-uniform: an utterance whose offsets contradict each other is skipped
    if (i0 < 0 || i1 > nS || i1 < i0 || !frames_ok(f0, f1, i1 - i0, nT)) return;
    const int64_t slot = (int64_t)blockIdx.x - (f0 / HB_RUN + b);
    const int64_t L = i1 - i0, T = f1 - f0;
    if (slot < 0 || slot * HB_RUN >= T) return;
    const int64_t j0 = slot * HB_RUN;                    // first hop block of the run
    const int64_t n0 = j0 * HB_HOP - HB_HALF;            // sample at xs[0]
    const float* xl = lo + i0;
    const float* xy = y16 + i0;
    for (int i = threadIdx.x; i < HB_SPAN; i += 256 * 3) {       // three loads of either signal in flight per thread
        f32x2 v[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int64_t n = n0 + i + 256 * u;
            const bool in = i + 256 * u < HB_SPAN && n >= 0 && n < L;
            v[u] = in ? f32x2{xl[n], xy[n]} : f32x2{0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 3; ++u)
            if (i + 256 * u < HB_SPAN) xs[i + 256 * u] = v[u];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int blk = wave * (HB_RUN / 4); blk < (wave + 1) * (HB_RUN / 4); ++blk) {
        if (j0 + blk >= T) break;                        // wave-uniform
        // samples s = blk 128 + 2 lane and s + 1 of the run; tap k of sample s reads xs[s + k].  One 16-byte read brings
        // two samples of both signals, and the pair a lane holds serves taps 2 j, 2 j + 1 of s and 2 j - 1, 2 j of s + 1
        const f32x4* p = reinterpret_cast<const f32x4*>(xs + blk * HB_HOP + 2 * lane);
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        f32x4 cur = p[0];
#pragma unroll
        for (int j = 0; j < HB_HALF; ++j) {
            const f32x4 nxt = p[j + 1];
            const float h0 = hp[2 * j], h1 = hp[2 * j + 1];
            a0 = fmaf(h0, cur.x, a0);
            b0 = fmaf(h0, cur.y, b0);
            a1 = fmaf(h0, cur.z, a1);
            b1 = fmaf(h0, cur.w, b1);
            a0 = fmaf(h1, cur.z, a0);
            b0 = fmaf(h1, cur.w, b0);
            a1 = fmaf(h1, nxt.x, a1);
            b1 = fmaf(h1, nxt.y, b1);
            cur = nxt;
        }
        const float hl = hp[TRUNET_HB_TAPS - 1];         // tap 62: the last pair, xs[s + 62] and xs[s + 63]
        a0 = fmaf(hl, cur.x, a0);
        b0 = fmaf(hl, cur.y, b0);
        a1 = fmaf(hl, cur.z, a1);
        b1 = fmaf(hl, cur.w, b1);
        // "same": the filter's tail past the utterance's last sample (the last block may be partial) does not count
        const int64_t n = (j0 + blk) * HB_HOP + 2 * lane;
        if (n >= L) a0 = b0 = 0.f;
        if (n + 1 >= L) a1 = b1 = 0.f;
        const float ex = wave_sum(fmaf(a1, a1, a0 * a0));
        const float ey = wave_sum(fmaf(b1, b1, b0 * b0));
        if (lane == 0) energy[f0 + j0 + blk] = f32x2{ex, ey};
    }
}

// grid (ceil(total_frames / 256)): frame t of an utterance sums the blocks t - 2 .. t + 1 that exist, j ascending
__global__ __launch_bounds__(256) void highband_gain_kernel(const f32x2* __restrict__ energy, const int64_t* __restrict__ so,
                                                            const int64_t* __restrict__ fo, float* __restrict__ g, int B,
                                                            int64_t nS, int64_t nT, float g_min) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nT) return;
    const int b = prefix_find(fo, B, f);
    const int64_t i0 = so[b], i1 = so[b + 1], f0 = fo[b], f1 = fo[b + 1];
    if (i0 < 0 || i1 > nS || i1 < i0 || !frames_ok(f0, f1, i1 - i0, nT) || f < f0 || f >= f1) return;
    const int64_t t = f - f0, T = f1 - f0;
    float ex = 0.f, ey = 0.f;
#pragma unroll
    for (int d = -2; d <= 1; ++d) {
        if (t + d < 0 || t + d >= T) continue;
        const f32x2 e = energy[f + d];
        ex += e.x;
        ey += e.y;
    }
    const float r = sqrtf((ey + HB_EPS) / (ex + HB_EPS));
    g[f] = fminf(fmaxf(r, g_min), 1.f);
}

// the gains of the samples n, n + 1, ..: c = (n pd) % D and t0 = (n pd) / D walk with the sample
struct hb_walk {
    const float* g;          // the utterance's T frame gains
    int last;                // T - 1
    int t0;
    unsigned c, pd, D;
    __device__ __forceinline__ float next() {
        const int ta = t0 < last ? t0 : last, tb = ta < last ? ta + 1 : last;
        // (1 - al) g[ta] + al g[tb], al = c / D, as (g[ta] (D - c) + g[tb] c) / D (highband_mix.hpp)
        const float G = hb_lerp(g[ta], g[tb], c, D);
        c += pd;
        if (c >= D) {        // pd < D: at most one frame per sample
            c -= D;
            ++t0;
        }
        return G;
    }
};

// grid (total_samples / HJ_TILE + B)
template <bool FOLLOW>
__global__ __launch_bounds__(256) void highband_join_kernel(const float* __restrict__ up_y, const float* __restrict__ up_x,
                                                            const float* __restrict__ x, const float* __restrict__ g,
                                                            float* __restrict__ out, const int64_t* __restrict__ so,
                                                            const int64_t* __restrict__ uo, const int64_t* __restrict__ fo,
                                                            int B, int64_t nS, int64_t nU, int64_t nT, int pd, int qd) {
    const int b = slot_find(so, B, (int64_t)blockIdx.x, HJ_TILE);
    const int64_t s0 = so[b], s1 = so[b + 1], u0 = uo[b], u1 = uo[b + 1];
    // workgroup-uniform: an utterance whose offsets contradict each other is skipped
    if (s0 < 0 || s1 > nS || s1 < s0 || u0 < 0 || u1 > nU || u1 - u0 < s1 - s0) return;
    const int64_t L = s1 - s0;
    const int64_t slot = (int64_t)blockIdx.x - (s0 / HJ_TILE + b);
    if (slot < 0 || slot * HJ_TILE >= L) return;
    const int64_t n0 = slot * HJ_TILE;                   // first sample of the tile
    const int cnt = (int)(L - n0 < HJ_TILE ? L - n0 : HJ_TILE);
    const unsigned D = (unsigned)HB_HOP * (unsigned)qd;
    int64_t tt = 0;
    unsigned ct = 0;
    const float* gb = g;
    int last = 0;
    if (FOLLOW) {
        const int64_t f0 = fo[b], f1 = fo[b + 1];
        if (!frames_ok(f0, f1, (L * pd + qd - 1) / qd, nT)) return;
        gb = g + f0;
        last = (int)(f1 - f0 - 1);
        const int64_t s = n0 * pd;                       // below 2^41
        tt = s / D;
        ct = (unsigned)(s - tt * D);
    }
    const float* py = up_y + u0 + n0;
    const float* pu = up_x + u0 + n0;
    const float* px = x + s0 + n0;
    float* po = out + s0 + n0;
    const bool vec_x = ((((uintptr_t)px) | ((uintptr_t)po)) & 15) == 0;
    const bool vec_u = ((((uintptr_t)py) | ((uintptr_t)pu)) & 15) == 0;
    for (int i = threadIdx.x * 4; i < cnt; i += 256 * 4) {
        hb_walk w = {gb, last, 0, 0u, (unsigned)pd, D};
        if (FOLLOW) {
            const unsigned c = ct + (unsigned)i * (unsigned)pd;          // below 128 * 640 + 4096 * 640
            const unsigned dt = c / D;
            w.c = c - dt * D;
            w.t0 = (int)(tt + dt);
        }
        if (i + 4 <= cnt) {
            const f32x4 vy = vec_u ? *reinterpret_cast<const f32x4*>(py + i) : f32x4{py[i], py[i + 1], py[i + 2], py[i + 3]};
            const f32x4 vu = vec_u ? *reinterpret_cast<const f32x4*>(pu + i) : f32x4{pu[i], pu[i + 1], pu[i + 2], pu[i + 3]};
            const f32x4 vx = vec_x ? *reinterpret_cast<const f32x4*>(px + i) : f32x4{px[i], px[i + 1], px[i + 2], px[i + 3]};
            f32x4 r;
            r.x = hb_mix<FOLLOW>(vy.x, vu.x, vx.x, FOLLOW ? w.next() : 1.f);
            r.y = hb_mix<FOLLOW>(vy.y, vu.y, vx.y, FOLLOW ? w.next() : 1.f);
            r.z = hb_mix<FOLLOW>(vy.z, vu.z, vx.z, FOLLOW ? w.next() : 1.f);
            r.w = hb_mix<FOLLOW>(vy.w, vu.w, vx.w, FOLLOW ? w.next() : 1.f);
            if (vec_x) {
                *reinterpret_cast<f32x4*>(po + i) = r;
            } else {
                po[i] = r.x;
                po[i + 1] = r.y;
                po[i + 2] = r.z;
                po[i + 3] = r.w;
            }
        } else {
            for (int k = i; k < cnt; ++k) po[k] = hb_mix<FOLLOW>(py[k], pu[k], px[k], FOLLOW ? w.next() : 1.f);
        }
    }
}

const int64_t HB_LIM = ((int64_t)1 << 31) - 1;

// sum (1 + L_b / 128) over B utterances of total_samples samples lies in [(total_samples + B) / 128, total_samples / 128 + B]
bool hb_frames_ok(int B, int64_t total_samples, int64_t total_frames) {
    return total_frames * HB_HOP >= total_samples + B && total_frames * HB_HOP <= total_samples + (int64_t)B * HB_HOP;
}

}  // namespace

extern "C" int trunet_highband_gains(const float* lo, const float* y16, const int64_t* sample_off, const int64_t* frame_off,
                                     const float* hp, float* energy, float* g, int B, int64_t total_samples,
                                     int64_t total_frames, float g_min, void* stream) {
    if (!lo || !y16 || !sample_off || !frame_off || !hp || !energy || !g || B < 1 || total_samples < 0 ||
        total_samples > HB_LIM || !hb_frames_ok(B, total_samples, total_frames) || !(g_min > 0.f) || !(g_min <= 1.f))
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(highband_energy_kernel, dim3((unsigned)(total_frames / HB_RUN + B)), dim3(256), 0, (hipStream_t)stream,
                       lo, y16, sample_off, frame_off, hp, reinterpret_cast<f32x2*>(energy), B, total_samples, total_frames);
    if (trunet_launch_status() != TRUNET_OK) return TRUNET_ELAUNCH;
    hipLaunchKernelGGL(highband_gain_kernel, dim3((unsigned)((total_frames + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const f32x2*>(energy), sample_off, frame_off, g, B, total_samples, total_frames, g_min);
    return trunet_launch_status();
}

extern "C" int trunet_highband_join(const float* up_y, const float* up_x, const float* x, const float* g, float* out,
                                    const int64_t* sample_off, const int64_t* up_off, const int64_t* frame_off, int B,
                                    int64_t total_samples, int64_t total_up, int64_t total_frames, int pd, int qd, int mode,
                                    void* stream) {
    if (!up_y || !up_x || !x || !out || !sample_off || !up_off || B < 1 || total_samples < 0 || total_up < total_samples ||
        total_up > HB_LIM || pd < 1 || qd <= pd || qd > HB_MAX_RATIO || (mode != TRUNET_HB_KEEP && mode != TRUNET_HB_FOLLOW))
        return TRUNET_EINVAL;
    // T_b = 1 + ceil(L_b pd / qd) / 128 with pd < qd: between B and total_samples / 128 + B frames
    if (mode == TRUNET_HB_FOLLOW &&
        (!g || !frame_off || total_frames < B || total_frames * HB_HOP > total_samples + (int64_t)B * HB_HOP))
        return TRUNET_EINVAL;
    if (total_samples == 0) return TRUNET_OK;
    const dim3 grid((unsigned)(total_samples / HJ_TILE + B));
    if (mode == TRUNET_HB_FOLLOW)
        hipLaunchKernelGGL(highband_join_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, up_y, up_x, x, g, out,
                           sample_off, up_off, frame_off, B, total_samples, total_up, total_frames, pd, qd);
    else
        hipLaunchKernelGGL(highband_join_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, up_y, up_x, x, g, out,
                           sample_off, up_off, frame_off, B, total_samples, total_up, total_frames, pd, qd);
    return trunet_launch_status();
}
