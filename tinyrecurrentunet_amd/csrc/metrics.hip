// Speech-quality metrics of B clean / estimate pairs of any lengths, packed back to back (evaluate.py):
//   * polyphase resampler (fs -> 10 kHz, Kaiser-windowed sinc, the closed form of scipy.signal.resample_poly)
//   * STOI / ESTOI: silent-frame removal, fused overlap-add + 512-point STFT + third-octave bands, 30-frame segments
//   * SI-SDR on the signals at their own rate
//   * the backward of STOI / ESTOI as a loss in the estimate (stoi_loss.py), which reads the forward's workspace
// Every buffer is sized by what the host knows from the lengths (frames BEFORE silence removal), so a call needs no
// device -> host copy: the kept-frame count K_b lives on the device only and the later kernels read it.  No float atomics:
// every per-utterance reduction runs in a fixed order inside that utterance's own workgroups, so an utterance's results are
// bit for bit independent of its batch-mates and their order.
#include "common.hpp"
#include "fft_common.hpp"

namespace {

constexpr int SF = 256;          // STOI frame (samples at 10 kHz)
constexpr int SHOP = 128;
constexpr int SNFFT = 512;
constexpr int SBINS = 257;
constexpr int NBAND = 15;
constexpr int NSEG = 30;         // frames per segment
constexpr int SEG_WG = 64;       // segments per workgroup of stoi_segments_kernel
constexpr int SDR_CHUNK = 16384; // samples per workgroup of si_sdr_partials_kernel
constexpr int MAX_HALF_TAPS = 4096;
constexpr double DEPS = 2.220446049250313e-16;   // np.finfo(np.float64).eps

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------- resampler
// grid (ceil(total_out / 256), nsig); signal plane y of in / out starts at y * total_in / y * total_out.
// y[m] = p sum_n h[m q - n p + L] x[n], taps outside [0, 2L] zero; h (2L + 1 taps, unit sum) staged in LDS.
__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            const int64_t* __restrict__ io, const int64_t* __restrict__ oo,
                                                            const float* __restrict__ taps, int half, int p, int q, int B,
                                                            int64_t nIn, int64_t nOut) {
    extern __shared__ float h[];
    const int ntaps = 2 * half + 1;
    for (int i = threadIdx.x; i < ntaps; i += 256) h[i] = taps[i];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nOut) return;
    const int b = prefix_find(oo, B, g);
    const int64_t i0 = io[b], i1 = io[b + 1], o0 = oo[b], o1 = oo[b + 1];
    if (i0 < 0 || i1 > nIn || i1 < i0 || o0 < 0 || o1 > nOut || o1 - o0 != ((i1 - i0) * p + q - 1) / q) return;
    if (g < o0 || g >= o1) return;
    const int64_t len = i1 - i0, m = g - o0;
    const float* x = in + (size_t)blockIdx.y * nIn + i0;
    int64_t n = (m * q + half) / p;                 // the largest n with a tap t >= 0
    int64_t t = m * q + half - n * p;
    if (n > len - 1) { t += (n - (len - 1)) * p; n = len - 1; }
    float acc = 0.f;
    for (; t < ntaps && n >= 0; t += p, --n) acc += h[t] * x[n];
    out[(size_t)blockIdx.y * nOut + g] = (float)p * acc;
}

// ---------------------------------------------------------------- STOI / ESTOI
// Per utterance b: R_b resampled samples (sig_off), F_b = |range(0, R_b - 256, 128)| analysis frames (frame_off), at most
// S_b = max(F_b - 30, 0) segments (seg_off) and ceil(S_b / 64) segment workgroups (chunk_off).  All four tables are
// checked against each other; an utterance that fails is skipped.
struct StoiUtt { int64_t s0, f0, g0, c0; int F, S; };

__device__ __forceinline__ bool stoi_utt(const int64_t* __restrict__ so, const int64_t* __restrict__ fo,
                                         const int64_t* __restrict__ go, const int64_t* __restrict__ co, int b, int64_t nS,
                                         int64_t nF, int64_t nG, int64_t nC, StoiUtt& u) {
    const int64_t s0 = so[b], s1 = so[b + 1];
    if (s0 < 0 || s1 > nS || s1 < s0 || s1 - s0 > 0x7fffffffLL) return false;
    const int64_t R = s1 - s0;
    const int64_t F = R > SF ? (R - SF + SHOP - 1) / SHOP : 0;
    const int64_t S = F > NSEG ? F - NSEG : 0;
    const int64_t f0 = fo[b], g0 = go[b], c0 = co[b];
    if (f0 < 0 || fo[b + 1] - f0 != F || fo[b + 1] > nF) return false;
    if (g0 < 0 || go[b + 1] - g0 != S || go[b + 1] > nG) return false;
    if (c0 < 0 || co[b + 1] - c0 != (S + SEG_WG - 1) / SEG_WG || co[b + 1] > nC) return false;
    u.s0 = s0; u.f0 = f0; u.g0 = g0; u.c0 = c0; u.F = (int)F; u.S = (int)S;
    return true;
}

struct StoiArgs {
    const float* sig;                    // (2, nS): clean, estimate at 10 kHz
    const int64_t *so, *fo, *go, *co;
    const float* win;                    // hann(258)[1:-1]
    const int* edges;                    // 16 bin indices: band k = [edges[k], edges[k+1])
    double* energy;                      // (nF)  frame energies of the clean signal, dB
    int* kept;                           // (nF)  kept frame indices, at the utterance's frame offset
    int* count;                          // (B)   K_b
    float* tob;                          // (2, nF, 15) band magnitudes of the STFT frames of x_sil / y_sil
    double* seg;                         // (2, nG) per segment: sum over bands of d (STOI), ESTOI score
    double *stoi, *estoi;                // (B)
    int64_t* segments;                   // (B)
    int B;
    int64_t nS, nF, nG, nC;
};

// one wave per analysis frame of the clean signal: e = 20 log10(||w x[i : i + 256]|| + eps); grid (ceil(nF / 4))
__global__ __launch_bounds__(256) void stoi_energy_kernel(StoiArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.nF) return;                                    // uniform over the wave
    const int b = prefix_find(a.fo, a.B, g);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || g < u.f0 || g >= u.f0 + u.F) return;
    const float* x = a.sig + u.s0 + (g - u.f0) * SHOP;
    double e = 0.0;
#pragma unroll
    for (int r = 0; r < SF / 64; ++r) {
        const int s = lane + 64 * r;
        const double v = (double)(a.win[s] * x[s]);
        e += v * v;
    }
    e = wave_sum_f64(e);
    if (lane == 0) a.energy[g] = 20.0 * log10(sqrt(e) + DEPS);
}

// one workgroup per utterance: threshold max(e) - 40 dB, then the kept frames in order (a block scan of the mask)
__global__ __launch_bounds__(256) void stoi_silence_kernel(StoiArgs a) {
    __shared__ double red[256];
    __shared__ int wc[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, blockIdx.x, a.nS, a.nF, a.nG, a.nC, u)) return;
    const double* e = a.energy + u.f0;
    double mx = -HUGE_VAL;
    for (int i = tid; i < u.F; i += 256) mx = fmax(mx, e[i]);
    red[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
        __syncthreads();
    }
    const double thr = red[0] - 40.0;
    int base = 0;
    for (int i0 = 0; i0 < u.F; i0 += 256) {
        const int i = i0 + tid;
        const bool keep = i < u.F && e[i] > thr;
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wc[w] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int v = 0; v < w; ++v) off += wc[v];
        if (keep) a.kept[u.f0 + off + before] = i;
        base += wc[0] + wc[1] + wc[2] + wc[3];
        __syncthreads();
    }
    if (tid == 0) a.count[blockIdx.x] = base;
}

// w[s] x_sil[j 128 + s] for STFT frame j < K_b - 1 of the silence-free signal: x_sil[j 128 + s] is
// f_j[s] + f_{j-1}[128 + s] (s < 128) or f_j[s] + f_{j+1}[s - 128], f_k = w x[src_k 128 : src_k 128 + 256] the k-th kept
// frame, f_{-1} = 0
__device__ __forceinline__ float sil_frame(const float* __restrict__ x, const float* __restrict__ win,
                                           const int* __restrict__ kept, int F, int j, int s) {
    const int sj = min(max(kept[j], 0), F - 1);
    float v = win[s] * x[sj * SHOP + s];
    if (s < SHOP) {
        if (j > 0) v += win[SHOP + s] * x[min(max(kept[j - 1], 0), F - 1) * SHOP + SHOP + s];
    } else {
        v += win[s - SHOP] * x[min(max(kept[j + 1], 0), F - 1) * SHOP + s - SHOP];
    }
    return win[s] * v;
}

// STFT frames j, j + 1 (j even, j < K_b - 1) of the silence-free signals, one workgroup per even frame slot (grid nF; the
// odd slots return).  Per signal, the two frames are the real and imaginary parts of one 512-point FFT: the frames of one
// signal share a transform, never clean and estimate, so an all-zero clean signal keeps exactly zero bands whatever the
// estimate (fp32 rounding of the Hermitian split would otherwise leak the estimate into it).
__global__ __launch_bounds__(256) void stoi_bands_kernel(StoiArgs a, const cpx* __restrict__ tw) {
    __shared__ cpx sa[SNFFT], sb[SNFFT];
    __shared__ float pw[2][SBINS + 3];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int b = prefix_find(a.fo, a.B, g);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || g < u.f0 || g >= u.f0 + u.F) return;
    const int K = min(a.count[b], u.F);
    const int j = (int)(g - u.f0);
    if ((j & 1) || j >= K - 1) return;                        // uniform over the workgroup
    const bool two = j + 1 < K - 1;
    const int* kept = a.kept + u.f0;
    for (int sig = 0; sig < 2; ++sig) {
        const float* x = a.sig + (size_t)sig * a.nS + u.s0;
        {
            const int s = tid;                                // 256 threads: one sample of each frame
            sa[s] = make_float2(sil_frame(x, a.win, kept, u.F, j, s), two ? sil_frame(x, a.win, kept, u.F, j + 1, s) : 0.f);
            sa[s + SF] = make_float2(0.f, 0.f);
        }
        const cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
        for (int k = tid; k < SBINS; k += 256) {
            cpx A, B2;
            split_pair(Z, k, SNFFT, A, B2);
            pw[0][k] = A.x * A.x + A.y * A.y;
            pw[1][k] = B2.x * B2.x + B2.y * B2.y;
        }
        __syncthreads();
        if (tid < 2 * NBAND) {
            const int f = tid / NBAND, k = tid - f * NBAND;
            if (f == 0 || two) {
                const int lo = min(max(a.edges[k], 0), SBINS), hi = min(max(a.edges[k + 1], lo), SBINS);
                double acc = 0.0;
                for (int i = lo; i < hi; ++i) acc += (double)pw[f][i];
                a.tob[((size_t)sig * a.nF + g + f) * NBAND + k] = (float)sqrt(acc);
            }
        }
        __syncthreads();                                      // sa / pw are rewritten for the estimate
    }
}

// SEG_WG consecutive segments of one utterance per workgroup (grid nC), one wave per segment.  Segment s covers STFT frames
// s .. s + 29 (pystoi's m = s + 30); the workgroup stages its frames plus the 29-frame halo of both signals in LDS.
__global__ __launch_bounds__(256) void stoi_segments_kernel(StoiArgs a) {
    __shared__ float tb[2][SEG_WG + NSEG - 1][NBAND];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t c = blockIdx.x;
    const int b = prefix_find(a.co, a.B, c);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || c < u.c0) return;
    const int nseg = min(a.count[b], u.F) - NSEG;             // K_b - 30 segments, when K_b - 1 >= 30
    const int s0 = (int)(c - u.c0) * SEG_WG;
    if (s0 >= nseg) return;
    const int s1 = min(s0 + SEG_WG, nseg);
    const int rows = s1 - s0 + NSEG - 1;                      // STFT frames s0 .. s1 + 28 <= K_b - 2
    for (int i = tid; i < 2 * rows * NBAND; i += 256) {
        const int sig = i / (rows * NBAND), r = (i / NBAND) % rows, k = i % NBAND;
        tb[sig][r][k] = a.tob[((size_t)sig * a.nF + u.f0 + s0 + r) * NBAND + k];
    }
    __syncthreads();
    const double clipc = 1.0 + 5.623413251903491;             // 1 + 10^(15/20)
    for (int s = s0 + w; s < s1; s += 4) {
        const int r0 = s - s0;
        // STOI: lane k < 15 takes band k
        const int k = min(lane, NBAND - 1);
        double nx = 0.0, ny = 0.0;
        for (int t = 0; t < NSEG; ++t) {
            const double xv = tb[0][r0 + t][k], yv = tb[1][r0 + t][k];
            nx += xv * xv;
            ny += yv * yv;
        }
        nx = sqrt(nx);
        ny = sqrt(ny) + DEPS;
        double mxs = 0.0, mys = 0.0;
        for (int t = 0; t < NSEG; ++t) {
            const double xv = tb[0][r0 + t][k];
            mxs += xv;
            mys += fmin((double)tb[1][r0 + t][k] * nx / ny, xv * clipc);
        }
        const double mx = mxs / NSEG, my = mys / NSEG;
        double sxx = 0.0, syy = 0.0, sxy = 0.0;
        for (int t = 0; t < NSEG; ++t) {
            const double xv = tb[0][r0 + t][k];
            const double dx = xv - mx, dy = fmin((double)tb[1][r0 + t][k] * nx / ny, xv * clipc) - my;
            sxx += dx * dx;
            syy += dy * dy;
            sxy += dx * dy;
        }
        const double d = lane < NBAND ? sxy / ((sqrt(sxx) + DEPS) * (sqrt(syy) + DEPS)) : 0.0;
        const double dsum = wave_sum_f64(d);
        // ESTOI rows: band k's mean and norm + eps, for both signals
        double rm[2], rn[2];
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            double m = 0.0;
            for (int t = 0; t < NSEG; ++t) m += tb[sig][r0 + t][k];
            m /= NSEG;
            double q = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double v = tb[sig][r0 + t][k] - m;
                q += v * v;
            }
            rm[sig] = m;
            rn[sig] = sqrt(q) + DEPS;
        }
        // ESTOI columns: lane t < 30 takes frame t of the row-normalised matrices
        const int t = min(lane, NSEG - 1);
        double xc[NBAND], yc[NBAND];
        double cmx = 0.0, cmy = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            const double m0 = __shfl(rm[0], kk), n0 = __shfl(rn[0], kk);
            const double m1 = __shfl(rm[1], kk), n1 = __shfl(rn[1], kk);
            xc[kk] = (tb[0][r0 + t][kk] - m0) / n0;
            yc[kk] = (tb[1][r0 + t][kk] - m1) / n1;
            cmx += xc[kk];
            cmy += yc[kk];
        }
        cmx /= NBAND;
        cmy /= NBAND;
        double qx = 0.0, qy = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            xc[kk] -= cmx;
            yc[kk] -= cmy;
            qx += xc[kk] * xc[kk];
            qy += yc[kk] * yc[kk];
        }
        double dot = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) dot += xc[kk] * yc[kk];
        const double col = lane < NSEG ? dot / ((sqrt(qx) + DEPS) * (sqrt(qy) + DEPS)) : 0.0;
        const double esum = wave_sum_f64(col);
        if (lane == 0) {
            a.seg[u.g0 + s] = dsum;
            a.seg[a.nG + u.g0 + s] = esum / NSEG;
        }
    }
}

// one workgroup per utterance: the means over its segments in a fixed order (1e-5 when K_b - 1 < 30, as pystoi)
__global__ __launch_bounds__(256) void stoi_finalize_kernel(StoiArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, blockIdx.x, a.nS, a.nF, a.nG, a.nC, u)) return;
    const int nseg = max(min(a.count[blockIdx.x], u.F) - NSEG, 0);
    double s0 = 0.0, s1 = 0.0;
    for (int i = tid; i < nseg; i += 256) {
        s0 += a.seg[u.g0 + i];
        s1 += a.seg[a.nG + u.g0 + i];
    }
    s0 = block_sum_f64(s0, red);
    s1 = block_sum_f64(s1, red);
    if (tid == 0) {
        a.stoi[blockIdx.x] = nseg > 0 ? s0 / ((double)nseg * NBAND) : 1e-5;
        a.estoi[blockIdx.x] = nseg > 0 ? s1 / nseg : 1e-5;
        a.segments[blockIdx.x] = nseg;
    }
}

// ---------------------------------------------------------------- SI-SDR
// per SDR_CHUNK samples of one utterance (grid nC): fp64 sums s, e, s s, e e, s e -> partials (nC, 5)
__global__ __launch_bounds__(256) void si_sdr_partials_kernel(const float* __restrict__ s, const float* __restrict__ e,
                                                              const int64_t* __restrict__ so, const int64_t* __restrict__ co,
                                                              double* __restrict__ partials, int B, int64_t nS,
                                                              int64_t nC) {
    __shared__ double red[256];
    const int64_t c = blockIdx.x;
    const int b = prefix_find(co, B, c);
    const int64_t s0 = so[b], s1 = so[b + 1], c0 = co[b];
    if (s0 < 0 || s1 > nS || s1 < s0 || c0 < 0 || co[b + 1] > nC || co[b + 1] - c0 != (s1 - s0 + SDR_CHUNK - 1) / SDR_CHUNK)
        return;
    if (c < c0 || c >= co[b + 1]) return;
    const int64_t i0 = s0 + (c - c0) * SDR_CHUNK, i1 = min(i0 + SDR_CHUNK, s1);
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const double x = s[i], y = e[i];
        v[0] += x;
        v[1] += y;
        v[2] += x * x;
        v[3] += y * y;
        v[4] += x * y;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double r = block_sum_f64(v[k], red);
        if (threadIdx.x == 0) partials[c * 5 + k] = r;
    }
}

// one thread per utterance: its chunks in order, then the means removed analytically
__global__ __launch_bounds__(256) void si_sdr_finalize_kernel(const double* __restrict__ partials,
                                                              const int64_t* __restrict__ so,
                                                              const int64_t* __restrict__ co, double* __restrict__ out,
                                                              int B, int64_t nS, int64_t nC) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t s0 = so[b], s1 = so[b + 1], c0 = co[b], c1 = co[b + 1];
    if (s0 < 0 || s1 > nS || s1 < s0 || c0 < 0 || c1 > nC || c1 - c0 != (s1 - s0 + SDR_CHUNK - 1) / SDR_CHUNK) return;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t c = c0; c < c1; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += partials[c * 5 + k];
    const double n = (double)(s1 - s0);
    const double sss = v[2] - v[0] * v[0] / n;      // <s, s>, <e, e>, <s, e> of the zero-mean signals
    const double see = v[3] - v[1] * v[1] / n;
    const double sse = v[4] - v[0] * v[1] / n;
    const double alpha = sse / sss;
    const double tgt = alpha * alpha * sss;          // ||alpha s||^2
    const double res = see - 2.0 * alpha * sse + tgt; // ||alpha s - e||^2
    out[b] = 10.0 * log10(tgt / res);
}

// ---------------------------------------------------------------- STOI / ESTOI loss: the backward (stoi_loss.py, section 3q)
// The loss is -(1 / B) sum_b s_b with s_b the STOI or ESTOI above; everything computed from the clean signal (the kept-frame
// list, its bands, the clip level) is a constant.  The forward is trunet_stoi_ragged itself, whose workspace the backward
// reads: kept, count, tob.  Four launches, each sized by the ragged tables; every sum has a fixed order, no atomics.
constexpr int SEGCELLS = NSEG * NBAND;   // cotangents one segment hands to its 30 frames

struct StoiBwdArgs {
    double* dseg;                        // (nG, 30, 15) per segment: d(segment score) / d tob_y[s + t][k]
    double* dtob;                        // (nF, 15)     d loss / d tob_y
    int* inv;                            // (nF)         analysis frame -> its slot in kept, -1 when dropped
    float* dframe;                       // (nF, 256)    w[s] * cotangent of STFT frame j of the silence-free estimate
    const float* gout;                   // (1) cotangent of the loss
    double scale;                        // -lambda / B
    int extended;
    float* grad;                         // (nS) d loss / d estimate at 10 kHz
};

// stoi_segments_kernel's grid and staging; one wave per segment writes the 30 x 15 cotangents of its estimate bands.
// STOI (lane k < 15 owns band k): u_t = y_t nx / ny, y'_t = min(u_t, c x_t) with the gradient on the branch the forward took
// (u_t <= c x_t: the first), d = sxy / ((sqrt sxx + eps)(sqrt syy + eps)).  ESTOI (lane t < 30 owns frame t): the column
// correlation back through the column and the row normalisation.  sqrt has derivative 0 at 0 throughout.
__global__ __launch_bounds__(256) void stoi_segments_bwd_kernel(StoiArgs a, StoiBwdArgs g) {
    __shared__ float tb[2][SEG_WG + NSEG - 1][NBAND];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t c = blockIdx.x;
    const int b = prefix_find(a.co, a.B, c);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || c < u.c0) return;
    const int nseg = min(a.count[b], u.F) - NSEG;
    const int s0 = (int)(c - u.c0) * SEG_WG;
    if (s0 >= nseg) return;
    const int s1 = min(s0 + SEG_WG, nseg);
    const int rows = s1 - s0 + NSEG - 1;
    for (int i = tid; i < 2 * rows * NBAND; i += 256) {
        const int sig = i / (rows * NBAND), r = (i / NBAND) % rows, k = i % NBAND;
        tb[sig][r][k] = a.tob[((size_t)sig * a.nF + u.f0 + s0 + r) * NBAND + k];
    }
    __syncthreads();
    const double clipc = 1.0 + 5.623413251903491;
    for (int s = s0 + w; s < s1; s += 4) {
        const int r0 = s - s0;
        double* out = g.dseg + (size_t)(u.g0 + s) * SEGCELLS;
        if (!g.extended) {
            if (lane >= NBAND) continue;
            const int k = lane;
            double nx = 0.0, sy = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k], yv = tb[1][r0 + t][k];
                nx += xv * xv;
                sy += yv * yv;
            }
            nx = sqrt(nx);
            const double rsy = sqrt(sy), ny = rsy + DEPS;
            double mxs = 0.0, mys = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k];
                mxs += xv;
                mys += fmin((double)tb[1][r0 + t][k] * nx / ny, xv * clipc);
            }
            const double mx = mxs / NSEG, my = mys / NSEG;
            double sxx = 0.0, syy = 0.0, sxy = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k];
                const double dx = xv - mx, dy = fmin((double)tb[1][r0 + t][k] * nx / ny, xv * clipc) - my;
                sxx += dx * dx;
                syy += dy * dy;
                sxy += dx * dy;
            }
            const double A = sqrt(sxx) + DEPS, rs = sqrt(syy), Bn = rs + DEPS;
            const double P = 1.0 / (A * Bn), Q = syy > 0.0 ? sxy / (A * Bn * Bn * rs) : 0.0;
            // h_t = d d / d y'_t on the unclipped cells (the mean removal is self-adjoint on sum-zero rows), hy = sum h_t y_t
            double hy = 0.0, hm = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k], yv = tb[1][r0 + t][k];
                const double uv = yv * nx / ny, cv = xv * clipc;
                hm += P * (xv - mx) - Q * (fmin(uv, cv) - my);
            }
            hm /= NSEG;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k], yv = tb[1][r0 + t][k];
                const double uv = yv * nx / ny, cv = xv * clipc;
                const double h = uv <= cv ? P * (xv - mx) - Q * (fmin(uv, cv) - my) - hm : 0.0;
                hy += h * yv;
            }
            const double al = nx / ny, be = sy > 0.0 ? hy * nx / (ny * ny * rsy) : 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double xv = tb[0][r0 + t][k], yv = tb[1][r0 + t][k];
                const double uv = yv * nx / ny, cv = xv * clipc;
                const double h = uv <= cv ? P * (xv - mx) - Q * (fmin(uv, cv) - my) - hm : 0.0;
                out[t * NBAND + k] = al * h - be * yv;
            }
            continue;
        }
        // ESTOI rows, as the forward: band k's mean, sqrt of the centred sum of squares, and that + eps
        const int k = min(lane, NBAND - 1);
        double rm[2], rq[2];
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            double m = 0.0;
            for (int t = 0; t < NSEG; ++t) m += tb[sig][r0 + t][k];
            m /= NSEG;
            double q = 0.0;
            for (int t = 0; t < NSEG; ++t) {
                const double v = tb[sig][r0 + t][k] - m;
                q += v * v;
            }
            rm[sig] = m;
            rq[sig] = sqrt(q);
        }
        const int t = min(lane, NSEG - 1);
        double xc[NBAND], yc[NBAND];
        double cmx = 0.0, cmy = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            const double m0 = __shfl(rm[0], kk), n0 = __shfl(rq[0], kk) + DEPS;
            const double m1 = __shfl(rm[1], kk), n1 = __shfl(rq[1], kk) + DEPS;
            xc[kk] = (tb[0][r0 + t][kk] - m0) / n0;
            yc[kk] = (tb[1][r0 + t][kk] - m1) / n1;
            cmx += xc[kk];
            cmy += yc[kk];
        }
        cmx /= NBAND;
        cmy /= NBAND;
        double qx = 0.0, qy = 0.0, dot = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            xc[kk] -= cmx;
            yc[kk] -= cmy;
            qx += xc[kk] * xc[kk];
            qy += yc[kk] * yc[kk];
        }
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) dot += xc[kk] * yc[kk];
        const double Ax = sqrt(qx) + DEPS, ry = sqrt(qy), Ay = ry + DEPS;
        const double live = lane < NSEG ? 1.0 / NSEG : 0.0;             // the segment score is the mean of the 30 columns
        const double U = live / (Ax * Ay), V = qy > 0.0 ? live * dot / (Ax * Ay * Ay * ry) : 0.0;
        // G[kk]: cotangent of the row-normalised estimate at (kk, t), after the adjoint of the column-mean removal
        double gm = 0.0;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            xc[kk] = U * xc[kk] - V * yc[kk];
            gm += xc[kk];
        }
        gm /= NBAND;
#pragma unroll
        for (int kk = 0; kk < NBAND; ++kk) {
            const double G = xc[kk] - gm;
            const double m1 = __shfl(rm[1], kk), r1 = __shfl(rq[1], kk), n1 = r1 + DEPS;
            const double cv = (double)tb[1][r0 + t][kk] - m1;          // the centred band value
            const double gsum = wave_sum_f64(G);                        // lanes >= 30 hold 0
            const double gc = wave_sum_f64(G * cv);
            const double v = (G - gsum / NSEG) / n1 - (r1 > 0.0 ? gc / (n1 * n1 * r1) * cv : 0.0);
            if (lane < NSEG) out[t * NBAND + kk] = v;
        }
    }
}

// one thread per (analysis frame slot j, band k): d loss / d tob_y[j][k] = factor * the cotangents of the up to 30 segments
// that hold STFT frame j, added with s ascending; factor = scale * gout / (segments * (15 | 1)).  The band-0 thread also
// writes the inverse of the kept-frame list for source frame j (a binary search: kept is ascending).
__global__ __launch_bounds__(256) void stoi_dtob_kernel(StoiArgs a, StoiBwdArgs g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nF * NBAND) return;
    const int64_t fr = i / NBAND;
    const int k = (int)(i - fr * NBAND);
    const int b = prefix_find(a.fo, a.B, fr);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || fr < u.f0 || fr >= u.f0 + u.F) return;
    const int K = min(a.count[b], u.F), nseg = K - NSEG;
    const int j = (int)(fr - u.f0);
    if (k == 0) {
        const int* kept = a.kept + u.f0;
        int lo = 0, hi = K;                                           // first slot with kept[slot] >= j
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (kept[mid] < j) lo = mid + 1; else hi = mid;
        }
        g.inv[fr] = lo < K && kept[lo] == j ? lo : -1;
    }
    double acc = 0.0;
    if (nseg > 0 && j <= K - 2) {
        for (int s = max(j - (NSEG - 1), 0); s <= min(j, nseg - 1); ++s)
            acc += g.dseg[(size_t)(u.g0 + s) * SEGCELLS + (j - s) * NBAND + k];
        acc *= g.scale * (double)g.gout[0] / ((double)nseg * (g.extended ? 1 : NBAND));
    }
    g.dtob[fr * NBAND + k] = acc;
}

// stoi_bands_kernel's grid and frame pairing, for the estimate alone: the transform again, dZ_k = (dtob / tob) Z_k on the
// bins of a band (0 where tob is 0) and 0 elsewhere, and the adjoint of the zero-padded real transform: frames j and j + 1
// come back as the real and imaginary parts of one inverse FFT of the Hermitian extension (dZ_k + conj dZ_{512-k}) / 2.
__global__ __launch_bounds__(256) void stoi_bands_bwd_kernel(StoiArgs a, StoiBwdArgs g, const cpx* __restrict__ tw) {
    __shared__ cpx sa[SNFFT], sb[SNFFT];
    __shared__ float rat[2][NBAND + 1];
    __shared__ int ed[NBAND + 1];
    const int tid = threadIdx.x;
    const int64_t fr = blockIdx.x;
    const int b = prefix_find(a.fo, a.B, fr);
    StoiUtt u;
    if (!stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) || fr < u.f0 || fr >= u.f0 + u.F) return;
    const int K = min(a.count[b], u.F);
    const int j = (int)(fr - u.f0);
    if (K <= NSEG || (j & 1) || j >= K - 1) return;               // uniform over the workgroup
    const bool two = j + 1 < K - 1;
    const int* kept = a.kept + u.f0;
    const float* x = a.sig + (size_t)a.nS + u.s0;
    sa[tid] = make_float2(sil_frame(x, a.win, kept, u.F, j, tid), two ? sil_frame(x, a.win, kept, u.F, j + 1, tid) : 0.f);
    sa[tid + SF] = make_float2(0.f, 0.f);
    if (tid < 2 * NBAND) {
        const int f = tid / NBAND, k = tid - f * NBAND;
        float r = 0.f;
        if (f == 0 || two) {
            const double t = (double)a.tob[((size_t)a.nF + fr + f) * NBAND + k];
            r = t > 0.0 ? (float)(g.dtob[(fr + f) * NBAND + k] / t) : 0.f;
        }
        rat[f][k] = r;
    }
    if (tid <= NBAND) ed[tid] = min(max(a.edges[tid], 1), SNFFT / 2);   // bins 1 .. 255: none is its own mirror
    cpx* Z = fft_lds_t<9, false>(sa, sb, tw);
    cpx* Cb = Z == sa ? sb : sa;
    for (int i = tid; i < SNFFT; i += 256) {
        const int k = i <= SNFFT / 2 ? i : SNFFT - i;
        int band = -1;
        for (int q = 0; q < NBAND; ++q)
            if (k >= ed[q] && k < max(ed[q + 1], ed[q])) band = q;
        cpx v = make_float2(0.f, 0.f);
        if (band >= 0) {
            cpx A, B2;
            split_pair(Z, k, SNFFT, A, B2);
            const float ra = 0.5f * rat[0][band], rb = 0.5f * rat[1][band];
            A = make_float2(ra * A.x, ra * A.y);
            B2 = make_float2(rb * B2.x, rb * B2.y);
            v = i == k ? make_float2(A.x - B2.y, A.y + B2.x) : make_float2(A.x + B2.y, B2.x - A.y);
        }
        Cb[i] = v;
    }
    const cpx* d = fft_lds_t<9, true>(Cb, Z, tw);
    const float ws = a.win[tid];
    g.dframe[(size_t)fr * SF + tid] = ws * d[tid].x;
    if (two) g.dframe[(size_t)(fr + 1) * SF + tid] = ws * d[tid].y;
}

// one thread per 10 kHz sample m of the estimate: the adjoint of sil_frame's windowing and of the overlap-add of the kept
// frames, as a gather.  m lies in the analysis frames m / 128 - 1 and m / 128; a kept one sits at slot k = inv[.] and puts m
// at n = 128 k + s of the silence-free signal, which STFT frames n / 128 - 1 and n / 128 read.
__global__ __launch_bounds__(256) void stoi_signal_bwd_kernel(StoiArgs a, StoiBwdArgs g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nS) return;
    const int b = prefix_find(a.so, a.B, i);
    StoiUtt u;
    float acc = 0.f;
    if (stoi_utt(a.so, a.fo, a.go, a.co, b, a.nS, a.nF, a.nG, a.nC, u) && i >= u.s0 && i - u.s0 < (int64_t)u.F * SHOP + SF) {
        const int K = min(a.count[b], u.F);
        const int m = (int)(i - u.s0);
        if (K > NSEG) {
            for (int fi = m / SHOP - 1; fi <= m / SHOP; ++fi) {
                if (fi < 0 || fi >= u.F) continue;
                const int s = m - fi * SHOP;
                const int k = g.inv[u.f0 + fi];
                if (k < 0 || k >= K) continue;
                const int n = k * SHOP + s;
                float dys = 0.f;
                for (int j = n / SHOP - 1; j <= n / SHOP; ++j)
                    if (j >= 0 && j <= K - 2) dys += g.dframe[(size_t)(u.f0 + j) * SF + n - j * SHOP];
                acc += a.win[s] * dys;
            }
        }
    }
    g.grad[i] = acc;
}

// adjoint of resample_poly_kernel as a gather per input sample: dx[n] = p sum_m h[m q - n p + L] dy[m] over the outputs m
// of the same utterance whose tap index lies in [0, 2L], m ascending.  grid (ceil(total_in / 256)).
__global__ __launch_bounds__(256) void resample_poly_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                                                const int64_t* __restrict__ io,
                                                                const int64_t* __restrict__ oo,
                                                                const float* __restrict__ taps, int half, int p, int q,
                                                                int B, int64_t nIn, int64_t nOut) {
    extern __shared__ float h[];
    const int ntaps = 2 * half + 1;
    for (int i = threadIdx.x; i < ntaps; i += 256) h[i] = taps[i];
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= nIn) return;
    const int b = prefix_find(io, B, g);
    const int64_t i0 = io[b], i1 = io[b + 1], o0 = oo[b], o1 = oo[b + 1];
    float acc = 0.f;
    if (i0 >= 0 && i1 <= nIn && i1 >= i0 && o0 >= 0 && o1 <= nOut && o1 - o0 == ((i1 - i0) * p + q - 1) / q && g >= i0 &&
        g < i1) {
        const int64_t np = (g - i0) * p, M = o1 - o0;
        const int64_t lo = np > half ? (np - half + q - 1) / q : 0;
        const int64_t hi = min((np + half) / q, M - 1);
        const float* y = gy + o0;
        for (int64_t m = lo; m <= hi; ++m) acc += h[m * q - np + half] * y[m];
    }
    gx[g] = (float)p * acc;
}

// out[0] = (float)(-mean_b score_b) in fp64, b ascending; out[1] = lambda * out[0]; loss_accum (may be null) += out[1]
__global__ void stoi_loss_value_kernel(const double* __restrict__ score, int B, float lambda, float* __restrict__ out,
                                       float* __restrict__ loss_accum) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += score[b];
    const float v = (float)(-(s / B));
    out[0] = v;
    out[1] = lambda * v;
    if (loss_accum) loss_accum[0] += lambda * v;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int trunet_resample_ragged(const float* in, float* out, const int64_t* in_off, const int64_t* out_off,
                                      const float* taps, int half, int p, int q, int B, int64_t total_in,
                                      int64_t total_out, int nsig, void* stream) {
    if (!in || !out || !in_off || !out_off || !taps || half < 0 || half > MAX_HALF_TAPS || p < 1 || p > 64 || q < 1 ||
        q > 64 || B <= 0 || nsig < 1 || nsig > 2 || total_in < 0 || total_out < 0 || total_in > ((int64_t)1 << 40))
        return TRUNET_EINVAL;
    // sum ceil(L_b p / q) lies in [total_in p / q, total_in p / q + B)
    if (total_out * q < total_in * p || total_out * q >= total_in * p + (int64_t)B * q) return TRUNET_EINVAL;
    if (total_out == 0) return TRUNET_OK;
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)((total_out + 255) / 256), nsig), dim3(256),
                       (2 * half + 1) * sizeof(float), ST, in, out, in_off, out_off, taps, half, p, q, B, total_in,
                       total_out);
    return trunet_launch_status();
}

static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t trunet_stoi_workspace_bytes(int B, int64_t total_frames, int64_t total_segments) {
    if (B <= 0 || total_frames < 0 || total_segments < 0) return 0;
    return align256(total_frames * sizeof(double)) + align256(total_frames * sizeof(int)) + align256(B * sizeof(int)) +
           align256(2 * total_frames * NBAND * sizeof(float)) + align256(2 * total_segments * sizeof(double));
}

extern "C" int trunet_stoi_ragged(const float* sig, const int64_t* sig_off, const int64_t* frame_off,
                                  const int64_t* seg_off, const int64_t* chunk_off, const float* window,
                                  const int* band_edges, const float* tw512, void* workspace, double* stoi, double* estoi,
                                  int64_t* segments, int B, int64_t total_samples, int64_t total_frames,
                                  int64_t total_segments, int64_t total_chunks, void* stream) {
    if (!sig || !sig_off || !frame_off || !seg_off || !chunk_off || !window || !band_edges || !tw512 || !workspace ||
        !stoi || !estoi || !segments || B <= 0 || total_samples < 0 || total_samples > ((int64_t)1 << 40))
        return TRUNET_EINVAL;
    // F_b <= R_b / 128, S_b <= F_b, ceil(S_b / 64) chunks
    if (total_frames < 0 || total_frames > total_samples / SHOP || total_frames > 0x7fffffffLL ||
        total_segments < 0 || total_segments > total_frames || total_chunks * SEG_WG < total_segments ||
        total_chunks * SEG_WG > total_segments + (int64_t)B * (SEG_WG - 1))
        return TRUNET_EINVAL;
    char* w = (char*)workspace;
    StoiArgs a;
    a.sig = sig; a.so = sig_off; a.fo = frame_off; a.go = seg_off; a.co = chunk_off; a.win = window; a.edges = band_edges;
    a.energy = (double*)w;   w += align256(total_frames * sizeof(double));
    a.kept = (int*)w;        w += align256(total_frames * sizeof(int));
    a.count = (int*)w;       w += align256(B * sizeof(int));
    a.tob = (float*)w;       w += align256(2 * total_frames * NBAND * sizeof(float));
    a.seg = (double*)w;
    a.stoi = stoi; a.estoi = estoi; a.segments = segments;
    a.B = B; a.nS = total_samples; a.nF = total_frames; a.nG = total_segments; a.nC = total_chunks;
    if (total_frames > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)((total_frames + 3) / 4)), dim3(256), 0, ST, a);
    }
    hipLaunchKernelGGL(stoi_silence_kernel, dim3(B), dim3(256), 0, ST, a);
    if (total_frames > 0) {
        hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)total_frames), dim3(256), 0, ST, a, (const cpx*)tw512);
    }
    if (total_chunks > 0) {
        hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)total_chunks), dim3(256), 0, ST, a);
    }
    hipLaunchKernelGGL(stoi_finalize_kernel, dim3(B), dim3(256), 0, ST, a);
    return trunet_launch_status();
}

extern "C" size_t trunet_stoi_loss_workspace_bytes(int B, int64_t total_frames, int64_t total_segments) {
    if (B <= 0 || total_frames < 0 || total_segments < 0) return 0;
    return align256(total_segments * SEGCELLS * sizeof(double)) + align256(total_frames * NBAND * sizeof(double)) +
           align256(total_frames * sizeof(int)) + align256(total_frames * SF * sizeof(float));
}

extern "C" int trunet_stoi_loss_bwd(const float* sig, const int64_t* sig_off, const int64_t* frame_off,
                                    const int64_t* seg_off, const int64_t* chunk_off, const float* window,
                                    const int* band_edges, const float* tw512, const void* fwd_workspace,
                                    void* bwd_workspace, const float* gout, double scale, int extended, float* grad, int B,
                                    int64_t total_samples, int64_t total_frames, int64_t total_segments,
                                    int64_t total_chunks, void* stream) {
    if (!sig || !sig_off || !frame_off || !seg_off || !chunk_off || !window || !band_edges || !tw512 || !fwd_workspace ||
        !bwd_workspace || !gout || !grad || B <= 0 || total_samples < 0 || total_samples > ((int64_t)1 << 40) ||
        !(scale == scale) || (extended != 0 && extended != 1))
        return TRUNET_EINVAL;
    if (total_frames < 0 || total_frames > total_samples / SHOP || total_frames > 0x7fffffffLL ||
        total_segments < 0 || total_segments > total_frames || total_chunks * SEG_WG < total_segments ||
        total_chunks * SEG_WG > total_segments + (int64_t)B * (SEG_WG - 1))
        return TRUNET_EINVAL;
    if (total_samples == 0) return TRUNET_OK;
    char* w = (char*)fwd_workspace;                             // trunet_stoi_ragged's layout
    StoiArgs a;
    a.sig = sig; a.so = sig_off; a.fo = frame_off; a.go = seg_off; a.co = chunk_off; a.win = window; a.edges = band_edges;
    a.energy = (double*)w;   w += align256(total_frames * sizeof(double));
    a.kept = (int*)w;        w += align256(total_frames * sizeof(int));
    a.count = (int*)w;       w += align256(B * sizeof(int));
    a.tob = (float*)w;       w += align256(2 * total_frames * NBAND * sizeof(float));
    a.seg = (double*)w;
    a.stoi = nullptr; a.estoi = nullptr; a.segments = nullptr;
    a.B = B; a.nS = total_samples; a.nF = total_frames; a.nG = total_segments; a.nC = total_chunks;
    char* v = (char*)bwd_workspace;
    StoiBwdArgs g;
    g.dseg = (double*)v;     v += align256(total_segments * SEGCELLS * sizeof(double));
    g.dtob = (double*)v;     v += align256(total_frames * NBAND * sizeof(double));
    g.inv = (int*)v;         v += align256(total_frames * sizeof(int));
    g.dframe = (float*)v;
    g.gout = gout; g.scale = scale; g.extended = extended; g.grad = grad;
    if (total_chunks > 0) {
        hipLaunchKernelGGL(stoi_segments_bwd_kernel, dim3((unsigned)total_chunks), dim3(256), 0, ST, a, g);
    }
    if (total_frames > 0) {
        hipLaunchKernelGGL(stoi_dtob_kernel, dim3((unsigned)((total_frames * NBAND + 255) / 256)), dim3(256), 0, ST, a, g);
        hipLaunchKernelGGL(stoi_bands_bwd_kernel, dim3((unsigned)total_frames), dim3(256), 0, ST, a, g, (const cpx*)tw512);
    }
    hipLaunchKernelGGL(stoi_signal_bwd_kernel, dim3((unsigned)((total_samples + 255) / 256)), dim3(256), 0, ST, a, g);
    return trunet_launch_status();
}

extern "C" int trunet_resample_ragged_bwd(const float* gout, float* gin, const int64_t* in_off, const int64_t* out_off,
                                          const float* taps, int half, int p, int q, int B, int64_t total_in,
                                          int64_t total_out, void* stream) {
    if (!gout || !gin || !in_off || !out_off || !taps || half < 0 || half > MAX_HALF_TAPS || p < 1 || p > 64 || q < 1 ||
        q > 64 || B <= 0 || total_in < 0 || total_out < 0 || total_in > ((int64_t)1 << 40))
        return TRUNET_EINVAL;
    if (total_out * q < total_in * p || total_out * q >= total_in * p + (int64_t)B * q) return TRUNET_EINVAL;
    if (total_in == 0) return TRUNET_OK;
    hipLaunchKernelGGL(resample_poly_bwd_kernel, dim3((unsigned)((total_in + 255) / 256)), dim3(256),
                       (2 * half + 1) * sizeof(float), ST, gout, gin, in_off, out_off, taps, half, p, q, B, total_in,
                       total_out);
    return trunet_launch_status();
}

extern "C" int trunet_stoi_loss_value(const double* scores, int B, float lambda, float* out, float* loss_accum,
                                      void* stream) {
    if (!scores || !out || B <= 0 || !(lambda == lambda)) return TRUNET_EINVAL;
    hipLaunchKernelGGL(stoi_loss_value_kernel, dim3(1), dim3(64), 0, ST, scores, B, lambda, out, loss_accum);
    return trunet_launch_status();
}

extern "C" int trunet_si_sdr_ragged(const float* clean, const float* estimate, const int64_t* sample_off,
                                    const int64_t* chunk_off, double* partials, double* out, int B, int64_t total_samples,
                                    int64_t total_chunks, void* stream) {
    if (!clean || !estimate || !sample_off || !chunk_off || !partials || !out || B <= 0 || total_samples < 0 ||
        total_chunks * SDR_CHUNK < total_samples || total_chunks * SDR_CHUNK > total_samples + (int64_t)B * (SDR_CHUNK - 1))
        return TRUNET_EINVAL;
    if (total_chunks > 0) {
        hipLaunchKernelGGL(si_sdr_partials_kernel, dim3((unsigned)total_chunks), dim3(256), 0, ST, clean, estimate,
                           sample_off, chunk_off, partials, B, total_samples, total_chunks);
    }
    hipLaunchKernelGGL(si_sdr_finalize_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, ST, partials, sample_off,
                       chunk_off, out, B, total_samples, total_chunks);
    return trunet_launch_status();
}
