// The attenuation limit (atten.py): out[n] = y[n] + g (x[n] - y[n]) at 16 kHz, directly behind the
// overlap-add, with y the route's enhanced sample, x the dry input sample at the same position and g = 10^(-L / 20).
//   atten_ragged_kernel   enhance: in place on the iSTFT output of the packed batch, one gain per utterance
//   atten_rows_kernel     AudioStream: in place on a hop per stream, the dry samples read from the streams' rings
//   stream_atten_kernel   StreamPool: a workgroup per listed session.  A hop becomes final four hops after it arrived, so
//                         a slot keeps a DRY LINE, the samples fed and not yet returned (three hops and 127 pending samples
//                         at most).  The kernel reads [dry line | packet] as one line, blends the call's outputs from its
//                         head, stores the rest and moves the slot's current gain on to its target -- over the first hop
//                         the session emits after a change, linearly (atten_ramp).
// Memory-bound, two floats per sample.  No atomics, nothing read back; a session's result does not depend, bit for bit, on
// the sessions that share the launch.  A record whose extents leave the buffers passed in is skipped, workgroup-uniformly,
// before any load or store.
#include "common.hpp"
#include "atten_blend.hpp"

namespace {

constexpr int ATT_INTS = TRUNET_ATT_INTS;
constexpr int ATT_LINE = TRUNET_ATT_DRY_LINE;        // floats of a slot's dry line
constexpr int ATT_HOP = 128;
constexpr int ATT_TILE = 1024;                       // samples a workgroup of the ragged kernel owns: four per thread
static_assert(ATT_LINE >= 4 * ATT_HOP, "three hops and 127 pending samples");

// grid (ceil(total / ATT_TILE)): sample n of the packed batch belongs to utterance b = prefix_find(sample_off, B, n)
__global__ __launch_bounds__(256) void atten_ragged_kernel(float* __restrict__ audio, const float* __restrict__ dry,
                                                           const float* __restrict__ gains,
                                                           const int64_t* __restrict__ sample_off, int B, int64_t total) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t n = (int64_t)blockIdx.x * ATT_TILE + threadIdx.x + 256 * u;
        if (n >= total) return;
        const int b = prefix_find(sample_off, B, n);
        if (sample_off[b] > n || sample_off[b + 1] <= n || sample_off[b + 1] > total) continue;      // a corrupt table
        audio[n] = atten_blend(audio[n], dry[n], gains[b]);
    }
}

// grid (ceil(rows n / 256)): out[r, i] with the dry sample dry[r, i], rows out_stride and dry_stride floats apart
__global__ __launch_bounds__(256) void atten_rows_kernel(float* __restrict__ out, const float* __restrict__ dry,
                                                         const float* __restrict__ gains, int rows, int n, int out_stride,
                                                         int dry_stride) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (int64_t)rows * n) return;
    const int r = (int)(v / n), i = (int)(v - (int64_t)r * n);
    float* po = out + (size_t)r * out_stride + i;
    *po = atten_blend(*po, dry[(size_t)r * dry_stride + i], gains[r]);
}

struct att_ext {             // what the entry point was given: every record is held against it
    int n_sess, slots, n_packet, n_out;
};

struct att_rec {
    int slot, c0, poff, n, ooff, m, flags;
};

__device__ __forceinline__ bool att_span_ok(int off, int n, int total) {
    return off >= 0 && n >= 0 && n <= total && off <= total - n;
}

// record i of the plan, and whether it stays inside the extents (uniform over the workgroup that asks)
__device__ __forceinline__ bool att_load(const int32_t* __restrict__ plan, int i, const att_ext& e, att_rec& c) {
    const int32_t* r = plan + (size_t)i * ATT_INTS;
    c = {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
    if (c.slot < 0 || c.slot >= e.slots || (c.flags & ~(TRUNET_ATT_FIRST | TRUNET_ATT_CLOSING))) return false;
    if (c.c0 < 0 || c.c0 >= ATT_LINE || !att_span_ok(c.poff, c.n, e.n_packet) || !att_span_ok(c.ooff, c.m, e.n_out))
        return false;
    const int64_t keep = (int64_t)c.c0 + c.n - c.m;      // what the line holds after the call
    return (c.flags & TRUNET_ATT_CLOSING) ? keep == 0 : (keep >= 0 && keep < ATT_LINE);
}

// grid (n_sess)
__global__ __launch_bounds__(256) void stream_atten_kernel(float* __restrict__ out, float* __restrict__ dry_line,
                                                           float* __restrict__ g_cur, const float* __restrict__ g_tgt,
                                                           const float* __restrict__ packet,
                                                           const int32_t* __restrict__ plan, att_ext e) {
    __shared__ float stage[ATT_LINE];
    att_rec c;
    if (!att_load(plan, (int)blockIdx.x, e, c)) return;
    float* dl = dry_line + (size_t)c.slot * ATT_LINE;
    const float* pk = packet + c.poff;                   // read below n only: never when the call brought no samples
    float* po = out + c.ooff;
    const bool first = (c.flags & TRUNET_ATT_FIRST) != 0;
    const float tgt = g_tgt[c.slot];
    const float cur = first ? tgt : g_cur[c.slot];       // frame 0: the session starts at its own target
    for (int k = threadIdx.x; k < c.m; k += 256) {
        const float x = k < c.c0 ? dl[k] : pk[k - c.c0];
        const float g = (k < ATT_HOP && cur != tgt) ? atten_ramp(cur, tgt, k) : tgt;
        po[k] = atten_blend(po[k], x, g);
    }
    if (c.flags & TRUNET_ATT_CLOSING) return;            // nothing of the slot is kept
    const int keep = c.c0 + c.n - c.m;
    for (int k = threadIdx.x; k < keep; k += 256) {
        const int j = c.m + k;
        stage[k] = j < c.c0 ? dl[j] : pk[j - c.c0];
    }
    __syncthreads();                                     // every read of the line lies before this barrier
    for (int k = threadIdx.x; k < keep; k += 256) dl[k] = stage[k];
    if (threadIdx.x == 0 && (first || c.m > 0)) g_cur[c.slot] = tgt;
}

const int64_t ATT_LIM = ((int64_t)1 << 31) - 1;

}  // namespace

extern "C" int trunet_atten_blend_ragged(float* audio, const float* dry, const float* gains, const int64_t* sample_off, int B,
                                         int64_t total_samples, void* stream) {
    if (!audio || !dry || !gains || !sample_off || B < 1 || total_samples < (int64_t)B * 257 ||
        total_samples > ATT_LIM * (int64_t)ATT_TILE)
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(atten_ragged_kernel, dim3((unsigned)((total_samples + ATT_TILE - 1) / ATT_TILE)), dim3(256), 0,
                       (hipStream_t)stream, audio, dry, gains, sample_off, B, total_samples);
    return trunet_launch_status();
}

extern "C" int trunet_atten_blend_rows(float* out, const float* dry, const float* gains, int rows, int n, int out_stride,
                                       int dry_stride, void* stream) {
    if (!out || !dry || !gains || rows < 1 || n < 1 || out_stride < n || dry_stride < n ||
        (int64_t)rows * (out_stride > dry_stride ? out_stride : dry_stride) > ATT_LIM)
        return TRUNET_EINVAL;
    hipLaunchKernelGGL(atten_rows_kernel, dim3((unsigned)(((int64_t)rows * n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, out, dry, gains, rows, n, out_stride, dry_stride);
    return trunet_launch_status();
}

extern "C" int trunet_stream_atten(float* out, float* dry_line, float* g_cur, const float* g_tgt, const float* packet,
                                   const int32_t* plan, int n_sess, int slots, int n_packet, int n_out, void* stream) {
    if (!dry_line || !g_cur || !g_tgt || !plan || n_sess < 1 || slots < 1 || n_packet < 0 || n_out < 0 ||
        (n_packet > 0 && !packet) || (n_out > 0 && !out))
        return TRUNET_EINVAL;
    const att_ext e = {n_sess, slots, n_packet, n_out};
    hipLaunchKernelGGL(stream_atten_kernel, dim3((unsigned)n_sess), dim3(256), 0, (hipStream_t)stream, out, dry_line, g_cur,
                       g_tgt, packet, plan, e);
    return trunet_launch_status();
}
