// Time-domain loss terms of the train step: the segmental cosine-similarity loss of cos_loss.py:4-56 in
// its repaired form R8, and an SI-SDR loss, as three launches next to the fused loss tail of util._FusedLossFn.
//
//   wave_loss_partials_kernel   grid (work items, rows): one pass over audio and clean; per (row, segment, piece of at most
//                               TRUNET_WAVE_LOSS_PIECE samples) the fp64 sums  sum xy, sum xx, sum yy, sum x, sum y
//   wave_loss_finalize_kernel   one workgroup: the pieces of each (row, segment) summed in table order, the per-row terms,
//                               the coefficients (A, B, C) of  d loss / d audio = A clean + B audio + C  per (row, segment),
//                               and the reduction over rows and segments in a fixed order
//   wave_loss_grad_kernel       grid (row chunks, rows): g += g_loss[0] * (A clean + B audio + C) over the segments that
//                               contain each sample
//
// No atomics anywhere: every sum has one owner and a fixed order, so results repeat bit for bit, and a row's partial sums,
// terms and coefficients are functions of that row alone.  Everything the kernels index with comes from device tables the
// caller built; each kernel re-checks what it reads (segment inside [0, L], piece inside its segment, item lists consistent)
// and skips a segment that fails: a bad table costs a term, never an access outside the rows.
#include "common.hpp"

namespace {

constexpr int WP = TRUNET_WAVE_LOSS_PIECE;
constexpr int NQ = 5;                       // sum xy, sum xx, sum yy, sum x, sum y
constexpr int MAXSEG = TRUNET_WAVE_LOSS_MAX_SEG;

struct WaveDesc {
    const float* x;          // audio (B, L)
    const float* y;          // clean (B, L)
    const int* bounds;       // (nseg + 1)
    const int* seg_first;    // (nseg + 2)
    const int* items;        // (n_items, 2) = segment, piece
    int B, L, nseg, n_items;
    int vec;                 // rows are 16-byte aligned: L % 4 == 0 and aligned bases
};

struct WaveFin {
    double cos_lambda, si_lambda, cos_eps, si_eps;
    float* vals;
    float* terms;
    float* coef;
    float* loss_accum;
};

// [s, e) of segment seg; segment nseg is the SI-SDR pseudo-segment [0, L)
__device__ __forceinline__ bool seg_range(const int* bounds, int seg, int nseg, int L, int& s, int& e) {
    if (seg < 0 || seg > nseg) return false;
    if (seg == nseg) {
        s = 0;
        e = L;
        return true;
    }
    s = bounds[seg];
    e = bounds[seg + 1];
    return s >= 0 && s <= e && e <= L;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ void accum(double* acc, float xf, float yf) {
    const double x = xf, y = yf;            // the product of two fp32 values is exact in fp64
    acc[0] += x * y;
    acc[1] += x * x;
    acc[2] += y * y;
    acc[3] += x;
    acc[4] += y;
}

__global__ __launch_bounds__(256) void wave_loss_partials_kernel(const WaveDesc d, double* __restrict__ part) {
    const int item = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    double acc[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int seg = d.items[2 * item], piece = d.items[2 * item + 1];
    int s, e;
    if (seg_range(d.bounds, seg, d.nseg, d.L, s, e) && piece >= 0 && piece <= (e - s - 1) / WP && e > s) {
        const int lo = s + piece * WP, hi = min(lo + WP, e);
        const float* __restrict__ x = d.x + (size_t)b * d.L;
        const float* __restrict__ y = d.y + (size_t)b * d.L;
        if (d.vec) {
            // [lo, alo) scalar head, [alo, ahi) whole aligned quads, [ahi, hi) scalar tail (each under 4 samples)
            const int alo = min((lo + 3) & ~3, hi), ahi = max(hi & ~3, alo);
            if (t < alo - lo) accum(acc, x[lo + t], y[lo + t]);
            for (int i = alo + 4 * t; i < ahi; i += 4 * 256) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + i);
                const f32x4 yv = *reinterpret_cast<const f32x4*>(y + i);
                accum(acc, xv.x, yv.x);
                accum(acc, xv.y, yv.y);
                accum(acc, xv.z, yv.z);
                accum(acc, xv.w, yv.w);
            }
            if (t < hi - ahi) accum(acc, x[ahi + t], y[ahi + t]);
        } else {
            for (int i = lo + t; i < hi; i += 256) accum(acc, x[i], y[i]);
        }
    }
    // lanes of a wave through cross-lane moves, the four waves through one LDS slot each and one barrier
    __shared__ double red[4][NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = wave_sum_f64(acc[q]);
    if ((t & 63) == 0) {
#pragma unroll
        for (int q = 0; q < NQ; q++) red[t >> 6][q] = acc[q];
    }
    __syncthreads();
    if (t < NQ) part[((size_t)b * d.n_items + item) * NQ + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(256) void wave_loss_finalize_kernel(const WaveDesc d, const WaveFin f,
                                                                 const double* __restrict__ part) {
    __shared__ double sm[256];
    const int t = threadIdx.x, m1 = d.nseg + 1;
    const double w = d.nseg > 0 ? 1.0 / ((double)d.nseg * (double)d.B) : 0.0;
    double acc_cos = 0.0, acc_si = 0.0;
    for (int p = t; p < d.B * m1; p += 256) {
        const int b = p / m1, j = p - b * m1;
        double term = 0.0, A = 0.0, Bc = 0.0, C = 0.0;
        int s = 0, e = 0, first = 0, cnt = 0;
        bool ok = seg_range(d.bounds, j, d.nseg, d.L, s, e);
        if (ok) {
            first = d.seg_first[j];
            cnt = d.seg_first[j + 1] - first;
            const int want = (e - s + WP - 1) / WP;
            ok = first >= 0 && cnt >= 0 && first <= d.n_items - cnt && (cnt == want || (j == d.nseg && cnt == 0));
            for (int k = 0; ok && k < cnt; k++) ok = d.items[2 * (first + k)] == j && d.items[2 * (first + k) + 1] == k;
        }
        if (ok) {
            double S[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0};
            const double* pp = part + ((size_t)b * d.n_items + first) * NQ;
            for (int k = 0; k < cnt; k++)
                for (int q = 0; q < NQ; q++) S[q] += pp[k * NQ + q];
            if (j < d.nseg) {
                if (cnt == 0) {
                    term = 1.0;                                    // empty segment: cos = 0, no gradient
                } else {
                    const double nx = sqrt(S[1]), ny = sqrt(S[2]);
                    const double cx = fmax(nx, f.cos_eps), cy = fmax(ny, f.cos_eps);
                    term = 1.0 - S[0] / (cx * cy);
                    A = f.cos_lambda * w * (-1.0 / (cx * cy));
                    if (nx > f.cos_eps) Bc = f.cos_lambda * w * (S[0] / (cx * cx * cy * nx));
                }
                acc_cos += term;
            } else if (cnt > 0) {
                const double n = (double)d.L, mx = S[3] / n, my = S[4] / n;
                const double Sxy = S[0] - S[3] * S[4] / n, Sxx = S[1] - S[3] * S[3] / n, Syy = S[2] - S[4] * S[4] / n;
                if (Syy > 0.0) {
                    const double alpha = Sxy / Syy, P = Sxy * alpha, N = Sxx - P;
                    const double k10 = 10.0 / 2.302585092994045684;
                    term = 10.0 * log10((P + f.si_eps) / (N + f.si_eps));
                    const double cy = k10 * (2.0 * alpha / (P + f.si_eps) + 2.0 * alpha / (N + f.si_eps));
                    const double cx = -2.0 * k10 / (N + f.si_eps);
                    const double sc = -f.si_lambda / (double)d.B;  // loss = -mean_b sisdr_b
                    A = sc * cy;
                    Bc = sc * cx;
                    C = -(A * my + Bc * mx);
                }
                acc_si += term;
            }
        }
        f.terms[p] = (float)term;
        f.coef[3 * (size_t)p] = (float)A;
        f.coef[3 * (size_t)p + 1] = (float)Bc;
        f.coef[3 * (size_t)p + 2] = (float)C;
    }
    const double tc = block_sum_f64(acc_cos, sm);
    const double ts = block_sum_f64(acc_si, sm);
    if (t == 0) {
        const double lcos = tc * w, msi = ts / (double)d.B;
        const double wc = f.cos_lambda * lcos, wsi = -f.si_lambda * msi;
        f.vals[0] = (float)(wc + wsi);
        f.vals[1] = (float)lcos;
        f.vals[2] = (float)msi;
        f.vals[3] = (float)wc;
        f.vals[4] = (float)wsi;
        if (f.loss_accum) f.loss_accum[0] += (float)(wc + wsi);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void wave_loss_grad_kernel(const WaveDesc d, const float* __restrict__ coef,
                                                             const float* __restrict__ g_loss, float* __restrict__ g) {
    constexpr int W = VEC ? 4 : 1;
    __shared__ int sb[MAXSEG + 1];
    const int t = threadIdx.x, b = blockIdx.y, nseg = d.nseg;
    if (nseg > 0) {
        for (int i = t; i <= nseg; i += 256) sb[i] = d.bounds[i];
        __syncthreads();
    }
    const int i0 = (blockIdx.x * 256 + t) * W;
    if (i0 >= d.L) return;
    const float gl = g_loss[0];
    const float* cf = coef + (size_t)b * (nseg + 1) * 3;
    const float As = cf[3 * nseg], Bs = cf[3 * nseg + 1], Cs = cf[3 * nseg + 2];
    // the last segment that starts at or before i0; the samples after it walk forward from there
    int j = 0;
    for (int hi = nseg; hi - j > 1;) {
        const int mid = (j + hi) >> 1;
        if (sb[mid] <= i0) j = mid; else hi = mid;
    }
    const size_t off = (size_t)b * d.L + i0;
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, yv = xv, gv = xv;      // the scalar instance uses component 0
    if (VEC) {
        xv = *reinterpret_cast<const f32x4*>(d.x + off);
        yv = *reinterpret_cast<const f32x4*>(d.y + off);
        gv = *reinterpret_cast<const f32x4*>(g + off);
    } else {
        xv[0] = d.x[off];
        yv[0] = d.y[off];
        gv[0] = g[off];
    }
#pragma unroll
    for (int u = 0; u < W; u++) {
        const int i = i0 + u;
        while (j < nseg && i >= sb[j + 1]) j++;
        float v = fmaf(As, yv[u], fmaf(Bs, xv[u], Cs));
        if (j < nseg && i >= sb[j]) v += fmaf(cf[3 * j], yv[u], cf[3 * j + 1] * xv[u]);
        gv[u] += gl * v;
    }
    if (VEC) *reinterpret_cast<f32x4*>(g + off) = gv;
    else g[off] = gv[0];
}

int max_items(int L, int nseg) { return 2 * ((L + WP - 1) / WP) + nseg; }

bool extents_ok(int B, int L, int nseg) {
    return B > 0 && B <= 65535 && L > 0 && L <= (1 << 30) && nseg >= 0 && nseg <= MAXSEG;
}

struct Span { const void* p; size_t n; bool out; };

// true when a buffer that is written overlaps any other buffer
bool any_overlap(const Span* s, int n) {
    for (int i = 0; i < n; i++)
        for (int k = i + 1; k < n; k++) {
            if (!s[i].p || !s[k].p || !(s[i].out || s[k].out)) continue;
            const uintptr_t x = (uintptr_t)s[i].p, y = (uintptr_t)s[k].p;
            if (x < y + s[k].n && y < x + s[i].n) return true;
        }
    return false;
}

bool args_ok(const trunet_wave_loss_args* a) {
    if (!a || !a->audio || !a->clean || !a->bounds || !a->seg_first || !a->items) return false;
    if (!extents_ok(a->B, a->L, a->nseg)) return false;
    return a->n_items > 0 && a->n_items <= max_items(a->L, a->nseg);
}

WaveDesc make_desc(const trunet_wave_loss_args* a, const void* extra) {
    WaveDesc d;
    d.x = a->audio;
    d.y = a->clean;
    d.bounds = a->bounds;
    d.seg_first = a->seg_first;
    d.items = a->items;
    d.B = a->B;
    d.L = a->L;
    d.nseg = a->nseg;
    d.n_items = a->n_items;
    d.vec = a->L % 4 == 0 && (((uintptr_t)a->audio | (uintptr_t)a->clean | (uintptr_t)extra) & 15) == 0;
    return d;
}

}  // namespace

extern "C" size_t trunet_wave_loss_workspace_bytes(int B, int L, int nseg) {
    if (!extents_ok(B, L, nseg)) return 0;
    return (size_t)B * max_items(L, nseg) * NQ * sizeof(double);
}

extern "C" int trunet_wave_loss_fwd(const trunet_wave_loss_args* a, void* ws, size_t ws_bytes, float* vals, float* terms,
                                    float* coef, float* loss_accum, void* stream) {
    if (!args_ok(a) || !ws || !vals || !terms || !coef || ((uintptr_t)ws & 7)) return TRUNET_EINVAL;
    if (!(a->cos_eps >= 0.0) || !(a->si_sdr_eps >= 0.0)) return TRUNET_EINVAL;
    const size_t need = trunet_wave_loss_workspace_bytes(a->B, a->L, a->nseg);
    if (ws_bytes < need) return TRUNET_EINVAL;
    const size_t sig = (size_t)a->B * a->L * sizeof(float), rows = (size_t)a->B * (a->nseg + 1) * sizeof(float);
    const Span sp[] = {{a->audio, sig, false}, {a->clean, sig, false}, {a->bounds, (size_t)(a->nseg + 1) * 4, false},
                       {a->seg_first, (size_t)(a->nseg + 2) * 4, false}, {a->items, (size_t)a->n_items * 8, false},
                       {ws, need, true}, {vals, 5 * sizeof(float), true}, {terms, rows, true}, {coef, 3 * rows, true},
                       {loss_accum, sizeof(float), true}};
    if (any_overlap(sp, sizeof(sp) / sizeof(sp[0]))) return TRUNET_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const WaveDesc d = make_desc(a, nullptr);
    const WaveFin f = {a->cos_lambda, a->si_sdr_lambda, a->cos_eps, a->si_sdr_eps, vals, terms, coef, loss_accum};
    hipLaunchKernelGGL(wave_loss_partials_kernel, dim3(a->n_items, a->B), dim3(256), 0, st, d, (double*)ws);
    hipLaunchKernelGGL(wave_loss_finalize_kernel, dim3(1), dim3(256), 0, st, d, f, (const double*)ws);
    return trunet_launch_status();
}

extern "C" int trunet_wave_loss_grad(const trunet_wave_loss_args* a, const float* coef, const float* g_loss, float* g_audio,
                                     void* stream) {
    if (!args_ok(a) || !coef || !g_loss || !g_audio) return TRUNET_EINVAL;
    const size_t sig = (size_t)a->B * a->L * sizeof(float), rows = (size_t)a->B * (a->nseg + 1) * sizeof(float);
    const Span sp[] = {{a->audio, sig, false}, {a->clean, sig, false}, {a->bounds, (size_t)(a->nseg + 1) * 4, false},
                       {coef, 3 * rows, false}, {g_loss, sizeof(float), false}, {g_audio, sig, true}};
    if (any_overlap(sp, sizeof(sp) / sizeof(sp[0]))) return TRUNET_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const WaveDesc d = make_desc(a, g_audio);
    if (d.vec)
        hipLaunchKernelGGL(wave_loss_grad_kernel<true>, dim3((a->L / 4 + 255) / 256, a->B), dim3(256), 0, st, d, coef, g_loss,
                           g_audio);
    else
        hipLaunchKernelGGL(wave_loss_grad_kernel<false>, dim3((a->L + 255) / 256, a->B), dim3(256), 0, st, d, coef, g_loss,
                           g_audio);
    return trunet_launch_status();
}
