/*
 * trunet_hip.h -- C ABI of libtrunet_hip.so: the MI355X (gfx950) hot path of TRU-Net.
 *
 * The reference (Okrio/tinyrecurrentunet) has no FFI: its hot path is plain PyTorch module
 * calls.  Every entry point below replaces the ATen/cuDNN/cuFFT work behind one reference
 * call site (cited per function as file:line of /root/reference).  Conventions:
 *   - extern "C", plain pointers + sizes, no torch types; all pointers are DEVICE pointers
 *     unless named h_*; every call is asynchronous on `stream` (a hipStream_t passed as void*).
 *   - returns 0 on success, a negative TRUNET_E* code otherwise; never throws, never
 *     allocates or frees caller memory, keeps no global mutable state.
 *   - all arithmetic is fp32 ("f32"); BatchNorm statistics are reduced in fp64.  The trunet_bf16_* family at the end
 *     (BASELINE.json configs[2]) stores activations / their gradients as bf16 and multiplies on the bf16 MFMA with fp32
 *     accumulation; everything else about it (statistics, coefficients, weight gradients) stays fp32.
 *
 * Internal activation layout ("frames-last"): a tensor of C channels x L positions for N frames
 * is stored as float[C][L][NP] with NP = N rounded up to a multiple of 128 (the host engine pads to 256, the widest
 * conv_gemm tile); element
 * (c,l,n) lives at ((c*L + l)*NP + n).  Frames (the batch axis of network.py) are the contiguous
 * axis, so every conv tap / stride / pad / crop of network.py becomes a whole-row offset.
 */
#ifndef TRUNET_HIP_H
#define TRUNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRUNET_OK 0
#define TRUNET_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define TRUNET_ELAUNCH (-2)  /* HIP launch failure */
#define TRUNET_ENOTSUP (-3)  /* configuration outside what the kernels were built for */

#define TRUNET_TILE_FRAMES 128
#define TRUNET_MAX_SEG 5

/* B-operand prologue applied while staging rows into LDS */
enum { TRUNET_PRO_NONE = 0,   /* v                                   */
       TRUNET_PRO_BNRELU = 1, /* max(v*c0[ch] + c1[ch], 0)            (BatchNorm1d+ReLU, network.py:31-32) */
       TRUNET_PRO_BNBWD = 2   /* c0[ch]*v + c1[ch]*v2 + c2[ch]        (BatchNorm backward, v=dy, v2=z)     */ };

/* One K-segment of an implicit GEMM row: `nchan` channel rows of a frames-last tensor taken at
 * position q(p) = (p*pos_mul + pos_off)/pos_div (segment skipped when q is fractional/out of range). */
typedef struct {
    const float* src0;  /* [nchan][L][NP] */
    const float* src1;  /* second tensor for TRUNET_PRO_BNBWD, same shape; else NULL */
    const float* c0;    /* per-channel coefficient arrays (see prologue), may be NULL for PRO_NONE */
    const float* c1;
    const float* c2;
    int32_t nchan;
    int32_t L;
    int32_t pos_mul, pos_off, pos_div;
    int32_t woff;       /* weight offset of this segment: A(m,c) = W[(m+w_m_off)*ldw_m + c*ldw_c + woff] */
    int32_t mode;       /* TRUNET_PRO_* */
    int32_t _pad;
} trunet_seg;

enum { TRUNET_EPI_BIAS = 1,   /* add bias[m]                                                      */
       TRUNET_EPI_STATS = 2,  /* accumulate per-channel statistics into `partials`                 */
       TRUNET_EPI_ACCUM = 4,  /* add the value already stored at the output location               */
       TRUNET_EPI_MASK = 8,   /* multiply by [e0[m]*zmask + e1[m] > 0] (ReLU backward)              */
       TRUNET_EPI_RELU = 16,  /* max(.,0) before the store                                          */
       TRUNET_EPI_PREZERO = 64, /* with STATS: `partials` is already zero (trunet_bn_finalize_* leave the rows they consumed
                                   zero): the entry point skips its own zero-fill launch */
       TRUNET_EPI_F32OUT = 32 /* trunet_bf16_gemm only: `out` is an fp32 frames-last tensor [rows][out_L][NP] (the GRU input
                                 projection, whose consumer is the fp32 recurrence); with BIAS only               */ };

/* Implicit-GEMM conv (forward of Conv1d k=1 / ConvTranspose1d, and their data gradients):
 *   out[m][p+out_pos_off][n] = epi( sum_seg sum_c A_seg(m,c) * pro_seg(src_seg[c][q_seg(p)][n]) )
 * Replaces: nn.Conv1d(k=1) network.py:28,50,64,83,106; nn.ConvTranspose1d network.py:67,86,109;
 * F.pad + torch.cat network.py:96-98,116-118 (two segments, no copy); nn.GRU input projection
 * network.py:48; and the autograd backward of each.  Statistics (EPI_STATS): per channel
 * sum(v), sum(v*v) (forward BatchNorm) or, with EPI_MASK, sum(dy), sum(dy*(zmask-e2[m])) (BatchNorm
 * backward); one partial row per (workgroup, wave column group): partials[part][M_stat][2]. */
typedef struct {
    int32_t NP, N;            /* padded / valid frames */
    int32_t P, p_begin;       /* output positions p_begin .. p_begin+P-1 */
    int32_t M;                /* output channels of this launch (rows of A) */
    int32_t m_out_off;        /* channel offset in `out`, bias, e*, partials */
    int32_t out_L, out_pos_off;
    int32_t ldw_m, ldw_c, w_m_off;
    int32_t nseg;
    int32_t epi;              /* TRUNET_EPI_* flags */
    int32_t M_stat;           /* channel count of the statistics rows */
    float* out;               /* [*][out_L][NP] */
    const float* W;
    const float* bias;
    const float* zmask;       /* tensor shaped like out (EPI_MASK) */
    const float* e0; const float* e1; const float* e2;
    float* partials;          /* [nparts][M_stat][2] */
    trunet_seg seg[TRUNET_MAX_SEG];
} trunet_gemm_args;

/* number of partial rows a trunet_conv_gemm launch writes (so the caller can size `partials`) */
int trunet_conv_gemm_nparts(int M);
int trunet_conv_gemm(const trunet_gemm_args* h_args, void* stream);
/* The fp32 GEMMs on the bf16 matrix pipe (round 4): fp32 operands split into three bf16 terms (24 significand bits), six
 * v_mfma_f32_32x32x16_bf16 per 16 K-values with fp32 accumulation -- an fp32-grade result (error against float64 equal to
 * the fp32-MFMA kernels', tests/test_gemm_x3_gpu.py) at 6/16 of the fp32-MFMA time.  trunet_gemm_x3_enable(mask) selects
 * where (returns the previous mask; -1 only queries; environment TRUNET_GEMM_X3 = 0..3 sets the initial value):
 *   TRUNET_X3_BWD  (default ON)  the fused backward kernels trunet_pw_bwd (pw_bwd.hip) and trunet_convt_bwd
 *                  (convt_bwd.hip).  Backward is a linear map of the saved forward state: the forward pass, the loss and
 *                  the loss gradient stay bit for bit those of the fp32-MFMA path, the parameter gradients move at the 1e-7
 *                  level, and every parity gate of the fp32 path holds unchanged.
 *   TRUNET_X3_GEMM (default OFF) the launches of trunet_conv_gemm without a tensor-operand epilogue (no TRUNET_EPI_MASK /
 *                  ACCUM: the forward pass; one-tensor prologue, M = 64 or a multiple of 128, NP a multiple of 256) on
 *                  conv_gemm_x3_kernel (gemm_x3.hip).  Equally accurate, but the rounding pattern of the OUTPUT is then
 *                  uncorrelated with a sequential fp32 FMA chain, and the loss gradient of this network is ill conditioned
 *                  in a handful of output elements: at the benchmarked size the full-size gradient gate against the fp32
 *                  oracle does not hold, so it stays opt-in. */
#define TRUNET_X3_GEMM 1
#define TRUNET_X3_BWD 2
int trunet_gemm_x3_enable(int on);
/* launch geometry trunet_conv_gemm picks for these arguments (reporting): kernel instance
 * conv_gemm_kernel<rs, kc, two, epl, nw, nbt> (or conv_smallm_kernel<epl> when M <= 8 and !two), ring of nb LDS slots
 * (nbt = nb where the depth is a compile-time instance: !two, epl = 0, rs >= 2, nb 2 or 3; else 0);
 * nw = 8 (256-frame tiles, two waves per SIMD) needs NP to be a multiple of 256 */
int trunet_conv_gemm_plan(const trunet_gemm_args* h_args, int* rs, int* kc, int* nb, int* two, int* epl, int* nw);

/* Weight gradient of the same implicit GEMM (autograd of network.py:28,50,64,67,83,86,106,109,48):
 *   dW[(m+w_m_off)*ldw_m + c*ldw_c + woff_seg] = sum_{p,n<N} dz[m][p][n] * pro_seg(src_seg[c][q_seg(p)][n])
 * with dz = proA(a0[m][p][n], a1[m][p][n]).  Writes per-workgroup partial images of W (and of the
 * bias gradient sum_{p,n} dz) that trunet_reduce_partials sums. */
typedef struct {
    int32_t NP, N;
    int32_t P, p_begin;
    int32_t M;                 /* rows of dz handled by this launch (<=128) */
    int32_t a_L, a_pos_off;    /* dz tensors are [*][a_L][NP]; row position p + a_pos_off */
    int32_t a_m_off;           /* channel offset inside the dz tensors / coefficient arrays */
    int32_t a_mode;            /* TRUNET_PRO_NONE or TRUNET_PRO_BNBWD */
    int32_t ldw_m, ldw_c, w_m_off;
    int32_t nseg;
    int32_t w_numel;           /* elements of one partial W image */
    int32_t _pad;
    const float* a0; const float* a1;
    const float* ac0; const float* ac1; const float* ac2;
    float* w_partials;         /* [nparts][w_numel], ZERO-FILLED by the caller */
    float* b_partials;         /* [nparts][M_total_bias] or NULL */
    int32_t b_stride, b_off;   /* bias partial row length / channel offset */
    trunet_seg seg[TRUNET_MAX_SEG];
} trunet_wgrad_args;

int trunet_conv_wgrad_nparts(void);
int trunet_conv_wgrad(const trunet_wgrad_args* h_args, void* stream);

/* Fused backward of a Conv1d(k=1) layer in front of a BatchNorm (autograd of network.py:28,50,64,83 with the
 * F.pad/torch.cat of :96-98): ONE pass over (dy, z, sources) yields the weight/bias gradient partial images of
 * trunet_conv_wgrad AND, per source segment s, the data gradient
 *   g_s[c][q_s(p)][n] = sum_m W[m][woff_s + c] * dz[m][p][n]  (+ previous content of out)  (* [e0*zmask + e1 > 0])
 * with e0 = seg.c0, e1 = seg.c1 of the segment (1, 0 for TRUNET_PRO_NONE), plus the BatchNorm-backward statistics
 * sum(g_s), sum(g_s * (zmask - e2)) of that source: partials[trunet_pw_bwd_nparts()][nchan][2].
 * Restrictions (else TRUNET_ENOTSUP, use trunet_conv_gemm + trunet_conv_wgrad): w.a_mode = TRUNET_PRO_BNBWD,
 * every segment pos_mul = pos_div = 1, mode TRUNET_PRO_NONE or TRUNET_PRO_BNRELU and nchan % 32 == 0; M <= 32 (any M: the dz
 * block is padded to one 32-row MFMA tile) with sum nchan == 128; M in {64, 96, 128} with sum nchan in {64, 128}; M == 64 also
 * with sum nchan == 192, where no segment that reaches channels 128..191 may ask for statistics.  Every shape runs on
 * pw_bwd_kernel (pw_bwd.hip); rows M .. of the padded dz block count as zero.  (M <= 8 with nchan % 8 == 0 runs on a
 * vector-ALU kernel instead only when the environment has TRUNET_PWB_THIN_VALU=1, read once per process.)
 * What a launch writes: every element (m < M, c < nchan) of the weight in EVERY partial image and elements b_off .. b_off +
 * M - 1 of every bias row, whatever they held (no zero fill needed for this entry point), and nothing else of either;
 * out[s] at every position q_s(p) some p reaches, all NP frames of it: dz is zero for frames >= N, so the padding columns
 * receive 0, or with ACCUM the masked previous content; positions no p reaches keep their content.  The statistics leave
 * frames >= N out. */
enum { TRUNET_DG_STORE = 1,  /* write the data gradient of this segment to `out`          */
       TRUNET_DG_MASK = 2,   /* ReLU backward: multiply by [e0*zmask + e1 > 0]             */
       TRUNET_DG_STATS = 4,  /* BatchNorm-backward statistics of the source (needs MASK)   */
       TRUNET_DG_ACCUM = 8,  /* add the value already stored in `out` before masking       */
       TRUNET_DG_PREZERO = 16 /* with STATS: `partials` is already zero (see TRUNET_EPI_PREZERO) */ };
typedef struct {
    float* out;            /* [nchan][seg.L][NP] */
    const float* zmask;    /* raw tensor of the source, same shape: must BE the segment's src0 (the kernel takes the mask
                              and the statistics' z from the rows it has staged; anything else: TRUNET_ENOTSUP) */
    const float* e2;       /* per-channel mean of the source's BatchNorm (STATS) */
    float* partials;       /* [trunet_pw_bwd_nparts()][nchan][2], zero-filled by the call */
    int32_t flags; int32_t _pad;
} trunet_dgrad_out;
typedef struct {
    trunet_wgrad_args w;   /* weight-gradient half: same meaning as for trunet_conv_wgrad */
    const float* W;        /* the layer's weight, addressed like w (ldw_m, ldw_c, w_m_off, seg.woff) */
    trunet_dgrad_out dg[TRUNET_MAX_SEG];
} trunet_pwbwd_args;
int trunet_pw_bwd_nparts(void);
int trunet_pw_bwd(const trunet_pwbwd_args* h_args, void* stream);

/* Fused backward of a ConvTranspose1d(64 -> 64, k, stride s, padding s/2) + BatchNorm layer whose input is the
 * BatchNorm+ReLU of a raw tensor `src` (autograd of network.py:67,86 between the BatchNorms of :65,84 and :72,91): ONE pass
 * over (dy, z, src) instead of trunet_conv_wgrad + trunet_conv_gemm over K tap segments each.
 *   dz = ca dy + cb z + cc;   dW[ci][co][k] = sum_{q,n<N} a[ci][q][n] dz[co][q s - pad + k][n],  a = max(s_scale src + s_shift, 0)
 *   db[co] = sum_{p,n} dz;    dsrc[ci][q][n] = [a > 0] sum_{co,k} W[ci][co][k] dz[co][q s - pad + k][n]
 *   partials[trunet_convt_bwd_nparts()][Ci][2] = sum dsrc, sum dsrc (src - s_mean)   (for trunet_bn_finalize_bwd)
 * w_partials / b_partials: per-workgroup partial images as for trunet_conv_wgrad (image stride w_numel, native
 * (Ci, Co, K) weight layout; trunet_convt_bwd_nparts() == trunet_conv_wgrad_nparts() images).
 * TRUNET_ENOTSUP unless Ci = Co = 64 and (k, s) in {(3,1), (3,2), (5,2)} (decoder.0 .. decoder.4). */
typedef struct {
    int32_t NP, N, Lin, Lout, K, S, pad, Ci, Co;
    int32_t w_numel, b_stride, b_off;
    const float* dy; const float* z;                   /* [Co][Lout][NP] */
    const float* ca; const float* cb; const float* cc; /* [Co] BatchNorm-backward coefficients of z */
    const float* src;                                  /* [Ci][Lin][NP] raw tensor in front of the layer's BatchNorm+ReLU */
    const float* s_scale; const float* s_shift; const float* s_mean;   /* [Ci] */
    const float* W;                                    /* (Ci, Co, K) */
    float* dsrc;                                       /* [Ci][Lin][NP] */
    float* partials;                                   /* [nparts][Ci][2] */
    float* w_partials; float* b_partials;
} trunet_convt_bwd_args;
int trunet_convt_bwd_nparts(void);
int trunet_convt_bwd(const trunet_convt_bwd_args* h_args, void* stream);

/* out[i] (+)= sum_g partials[g][i]  (deterministic second stage of every split reduction) */
int trunet_reduce_partials(float* out, const float* partials, int nparts, int numel, int accumulate,
                           void* stream);

/* BatchNorm1d training statistics -> affine (network.py:31,39,51,65,72 ...; torch semantics:
 * biased variance for normalisation, unbiased for running_var, momentum 0.1, eps 1e-5).
 * partials: [nparts][C][2] = sum, sumsq.  Writes scale = gamma*rstd, shift = beta - mean*scale,
 * mean, rstd; updates running_mean / running_var in place when non-NULL (both or neither; count == 1 takes the biased
 * variance) and adds 1 to the int64 counter num_batches_tracked (BatchNorm1d's buffer) when non-NULL.  Both finalize calls
 * leave the partial rows they consumed exactly +0, and return TRUNET_EINVAL for C, nparts or count <= 0.
 * The variance is sumsq / count - mean^2, in double but from the producers' fp32 partial sums: its absolute error is up to
 * 2^-24 (sum_g |sumsq_g| + 2 |mean| sum_g |sum_g|) / count, i.e. about 3 x 2^-24 mean^2 ("What pins the
 * BatchNorm chain"). */
int trunet_bn_finalize_fwd(float* partials, int nparts, int C, double count, const float* gamma,
                           const float* beta, float eps, float momentum, float* running_mean,
                           float* running_var, float* scale, float* shift, float* mean, float* rstd,
                           int64_t* num_batches_tracked, void* stream);
/* eval mode: scale/shift from running statistics (TRUNET_EINVAL for C <= 0) */
int trunet_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, float* scale, float* shift, void* stream);
/* BatchNorm backward reduction: partials [nparts][C][2] = sum(dy), sum(dy*(z-mean)).
 * Writes dgamma, dbeta and the coefficients of dz = ca*dy + cb*z + cc. */
int trunet_bn_finalize_bwd(float* partials, int nparts, int C, double count, const float* gamma,
                           const float* mean, const float* rstd, float* dgamma, float* dbeta, float* ca,
                           float* cb, float* cc, void* stream);

/* ReLU / BatchNorm+ReLU backward at a block boundary (the stand-alone block classes of network.py:9-120 receive the
 * cotangent of their post-activation output): dy[C][L][NP] *= [scale[c] z + shift[c] > 0] in place (scale == shift == NULL:
 * [z > 0], network.py:14) for frames < N, 0 beyond; with mean/partials non-NULL also the BatchNorm-backward sums
 * partials[trunet_relu_bwd_stats_nparts()][C][2] = sum dy, sum dy (z - mean[c]) for trunet_bn_finalize_bwd. */
int trunet_relu_bwd_stats_nparts(void);
int trunet_relu_bwd_stats(float* dy, const float* z, const float* scale, const float* shift, const float* mean,
                          float* partials, int C, int L, int NP, int N, void* stream);

/* (N,C,L) <-> frames-last [C][L][NP] (zero-fills frames >= N) */
int trunet_to_frames_last(const float* x_ncl, float* y_clnp, int N, int C, int L, int NP, void* stream);
int trunet_from_frames_last(const float* x_clnp, float* y_ncl, int N, int C, int L, int NP, void* stream);
/* same, applying y = max(scale[c]*x + shift[c], relu ? 0 : -inf) (BatchNorm1d+ReLU of a block output, network.py:31-32) */
int trunet_from_frames_last_affine(const float* x_clnp, float* y_ncl, int N, int C, int L, int NP, const float* scale,
                                   const float* shift, int relu, void* stream);

/* StandardConv1d forward (network.py:9-21): Conv1d(Cin->Cout,k,s,padding=s/2)+ReLU, frames-last. */
int trunet_conv_first_fwd(const float* x, const float* w, const float* b, float* y, int Cin, int Cout,
                          int K, int S, int Lin, int Lout, int NP, void* stream);
/* (its weight gradient is trunet_conv_wgrad with one segment per tap, pos_mul = stride) */

/* Depthwise Conv1d (network.py:33-38, groups=C, padding=k/2) with BN+ReLU prologue on the input and
 * statistics of the raw output: partials [nparts][C][2].  (csrc/depthwise.hip, with the bf16 entry points below) */
int trunet_dwconv_fwd(const float* zin, const float* s_in, const float* t_in, const float* w,
                      const float* b, float* zout, float* partials, int C, int K, int S, int Lin, int Lout,
                      int NP, int N, void* stream);
int trunet_dwconv_nparts(int Lout);
/* Depthwise backward: dz = ca*dy + cb*z + cc (BN backward of the dw output), then
 *   g_in = conv_transpose(dz, w) masked by ReLU of the input BN -> dy_in (+ its BN-backward stats),
 *   dw[c][k], db[c] partials. */
int trunet_dwconv_bwd(const float* dy, const float* z, const float* ca, const float* cb, const float* cc,
                      const float* zin, const float* s_in, const float* t_in, const float* mean_in,
                      const float* w, float* dy_in, float* partials_in, float* w_partials,
                      float* b_partials, int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream);
/* The same without the z operand: z = bias + conv(act(zin), w) is recomputed from the input rows the kernel holds anyway,
 * in trunet_dwconv_fwd's order of operations (bit for bit the stored tensor): one row pass less over HBM.
 * TRUNET_ENOTSUP for (K, S, Lin, Lout) outside the sliding-window kernels' shapes: call trunet_dwconv_bwd then. */
int trunet_dwconv_bwd_rz(const float* dy, const float* bias, const float* ca, const float* cb, const float* cc,
                         const float* zin, const float* s_in, const float* t_in, const float* mean_in,
                         const float* w, float* dy_in, float* partials_in, float* w_partials,
                         float* b_partials, int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream);
int trunet_dwconv_bwd_nparts(int Lin);

/* Bidirectional GRU recurrence over L positions (nn.GRU, network.py:48,55; torch gate order r,z,n).
 * gi: [2*3H][L][NP] input projections (+b_ih), hout: [2H][L][NP]; gates (training, may be NULL):
 * [2][4][H][L][NP] = r, z, n, (W_hn h + b_hn). */
int trunet_gru_fwd(const float* gi, const float* w_hh, const float* b_hh, const float* w_hh_rev,
                   const float* b_hh_rev, float* hout, float* gates, int H, int L, int NP, void* stream);
/* BPTT: dhout [2H][L][NP] -> dgi [2*3H][L][NP], dgh_n [2][H][L][NP] (dgh for r,z equals dgi). */
int trunet_gru_bwd(const float* dhout, const float* hout, const float* gates, const float* w_hh,
                   const float* w_hh_rev, float* dgi, float* dghn, int H, int L, int NP, int N,
                   void* stream);

/* One time step of a unidirectional nn.GRU cell (the TGRU of network.py:150 in stateful streaming use):
 * gi = W_ih x + b_ih and gh = W_hh h + b_hh are [3H][L][NP] (two trunet_conv_gemm launches), h / h_new [H][L][NP];
 * torch gate order r, z, n; h_new = (1 - z) n + z h. */
int trunet_gru_cell(const float* gi, const float* gh, const float* h, float* h_new, int H, int L, int NP, void* stream);

/* ---- TGRU as a trained layer (network.py:150 used as drawn in docs/net.jpg; build-defined forward).
 * The time axis of the recurrence is the FRAME axis, so the block works on "sequence-major" tensors
 * y[c][t][s], s = b*Lf + l < S = B*Lf (padded to SP): every (utterance b, frequency position l) is one sequence.
 * to:   y = max(scale[c] x + shift[c], relu ? 0 : -inf) of frames-last x[c][l][b*T + t] (scale == NULL: y = x); y = 0 for s >= S
 * from: x = y (zsrc == NULL), or x = y * [scale z + shift > 0] with z = zsrc (same layout as x) and the BatchNorm-backward
 *       sums of x: partials[trunet_from_seq_major_nparts()][C][2] = sum x, sum x (z - mean[c]). */
int trunet_to_seq_major(const float* x, float* y, const float* scale, const float* shift, int relu, int C, int Lf, int T,
                        int B, int NP, int SP, void* stream);
int trunet_from_seq_major_nparts(int Lf, int T, int B);
int trunet_from_seq_major(const float* y, float* x, const float* zsrc, const float* scale, const float* shift,
                          const float* mean, float* partials, int C, int Lf, int T, int B, int NP, int SP, void* stream);
/* time step t of nn.GRU (torch gate order r, z, n) on sequence-major tensors: gi_all [3H][T][SP] = W_ih x + b_ih,
 * gh [3H][SP] = W_hh h_{t-1} + b_hh (trunet_conv_gemm), hs [H][T+1][SP] with h_{t} at position t+1 (position 0 = h_{-1} = 0),
 * gates [4][H][T][SP] = r, z, n, gh_n (NULL in eval).  bwd: dhs [H][T+1][SP] holds dL/dh_t at position t+1 and receives
 * the direct term dh_t z_t at position t; carry [H][SP] = W_hh^T dgh_{t+1} (NULL at t = T-1); writes dgi_all / dgh_all
 * [3H][T][SP] rows of step t; sequences s >= S carry no gradient. */
/* the same T forward steps as one persistent launch (H = 128): W_hh in registers, h through LDS; writes hs positions
 * 1..T (position 0 must hold h_{-1} = 0) and, when non-NULL, the gates.  Here gi_all must already include
 * b_ih + (b_hr, b_hz, 0) and b_hn points at the last H entries of b_hh (only b_hn sits inside r * (W_hn h + b_hn)). */
int trunet_tgru_rec_fwd(const float* gi_all, const float* w_hh, const float* b_hn, float* hs, float* gates, int H, int T,
                        int SP, void* stream);
/* the T backward steps as one persistent launch (H = 128): reads dhs positions 1..T (dL/dh_t from the block's conv),
 * hs, gates; writes dgi_all / dgh_all [3H][T][SP]; the carried gradient stays in registers (dhs is not modified). */
int trunet_tgru_rec_bwd(const float* dhs, const float* hs, const float* gates, const float* w_hh, float* dgi_all,
                        float* dgh_all, int H, int T, int SP, int S, void* stream);
int trunet_tgru_cell_fwd(const float* gi_all, const float* gh, float* hs, float* gates, int H, int T, int t, int SP,
                         void* stream);
int trunet_tgru_cell_bwd(float* dhs, const float* carry, const float* hs, const float* gates, float* dgi_all,
                         float* dgh_all, int H, int T, int t, int SP, int S, void* stream);

/* fused AdamW over a flat buffer (torch.optim.AdamW, train.py:68,140) */
int trunet_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                 float beta2, float eps, float wd, int step, void* stream);
/* sum of squares -> out[0] (clip_grad_norm_ total norm^2, train.py:138) */
int trunet_sumsq(const float* g, int64_t n, float* out, void* stream);
/* 64-bit content checksum of n device buffers in one launch: desc = n x {const void* ptr; int64_t nwords (32-bit words)} in
 * device memory, out[0] (zero on entry) receives the sum of the mixed words.  Host-side cache key of the folded eval
 * artefact (network.py:153-171 in eval mode): catches weights written through `p.data` (util.py:168-175). */
int trunet_checksum_batch(const void* desc, int n, uint64_t* out, void* stream);


/* ---- FFT-based front / back end (all sizes fp32; tw = exp(-2*pi*i*t/n), t < n/2, interleaved re,im) ---- */

/* ProcessAudio.forward (dataset.py:246-272): rectangular-window, centre/reflect STFT (n_fft 512, hop 128)
 * of B utterances -> feat (B*T, C, 257), T = 1 + L/128; C = 3: (norm-dB-mag, sin, cos) (dataset.py:268-270),
 * C = 4: channel 1 is left for trunet_pcen.  mag (B, T, 257) is written when non-NULL.
 * Two frames share one transform (here, in the _fl and ragged siblings: frames 2i, 2i+1 of an utterance; in
 * trunet_stream_features: streams 2i, 2i+1), so a frame's rounding error is proportional to its partner's norm as well as to
 * its own; a frame whose 512 samples are all exactly zero is exact whatever its partner holds: mag 0, nm -1, (sin, cos) =
 * (0, 1), as torch.stft has it. */
int trunet_stft_features(const float* audio, float* feat, float* mag, const float* tw512, int B, int L, int T,
                         int C, void* stream);
/* pcenfunc (dataset.py:56-76) on mag (B, T, 257); out points at channel 1 of feat, out_stride = C*257 */
int trunet_pcen(const float* mag, float* out, int B, int T, int out_stride, float eps, float s, float alpha,
                float delta, float r, void* stream);
/* R7 glue (util.py:217-235 intent; phm.py:31-45; dataset.py:182-203,293-296): net output (B*T, 8, 257) ->
 * phase-aware mask -> rect-window iSTFT -> audio (B, L), L = 128 (T-1).  frames: scratch (B, T, 512).
 * With clean != NULL also writes per-block sums of |audio - clean| (util.py:239) to l1_partials
 * (trunet_mask_istft_l1_nparts(B, L) = B * ceil(L / 256) floats; the last block of L = 128 * odd sums 128 samples).
 * Arguments: B >= 1, T >= 2, L == 128 (T-1); anything else is TRUNET_EINVAL before a launch.
 * Backward: a phase pair that is exactly (0, 0) gets gradient 0 (c2 = c3 = 0 zeroes g2, g3; c6 = c7 = 0 zeroes g6, g7),
 * clamp(c0, -1, 1) passes its gradient on the closed interval, channels 1, 4, 5 get 0. */
int trunet_mask_istft_fwd(const float* net_out, float* frames, float* audio, const float* clean,
                          float* l1_partials, const float* tw512, int B, int T, int L, float beta, void* stream);
int trunet_mask_istft_l1_nparts(int B, int L);
int trunet_mask_istft_bwd(const float* g_audio, const float* net_out, float* g_net, const float* tw512, int B,
                          int T, int L, float beta, void* stream);
/* The same stages against the layer kernels' own layout, so that a training step needs no transpose pass at the network's
 * boundary: x, net_out and g_net are frames-last [C][257][NP] with frame n = b T + t in the last dimension, N = B T <= NP,
 * NP a multiple of 256 (anything else is TRUNET_EINVAL, as are the arguments the siblings above refuse).  Every value is
 * bit for bit what the sibling followed / preceded by trunet_to_frames_last / trunet_from_frames_last gives.
 * trunet_stft_features_fl: x [C][257][NP]; columns n >= N of the channels it writes are zero; mag [257][NP] when non-NULL.
 * trunet_pcen_fl: mag [257][NP] -> out = channel 1 of x ([257][NP]); columns n >= N are written as zero.
 * trunet_mask_istft_fwd_fl: net_out [8][257][NP]; frames, audio, l1_partials as trunet_mask_istft_fwd.
 * trunet_mask_istft_bwd_fl: g_net [8][257][NP]; columns n >= N are written as zero. */
int trunet_stft_features_fl(const float* audio, float* x, float* mag, const float* tw512, int B, int L, int T, int C,
                            int NP, void* stream);
int trunet_pcen_fl(const float* mag, float* out, int B, int T, int NP, float eps, float s, float alpha, float delta,
                   float r, void* stream);
int trunet_mask_istft_fwd_fl(const float* net_out, float* frames, float* audio, const float* clean, float* l1_partials,
                             const float* tw512, int B, int T, int L, int NP, float beta, void* stream);
int trunet_mask_istft_bwd_fl(const float* g_audio, const float* net_out, float* g_net, const float* tw512, int B, int T,
                             int L, int NP, float beta, void* stream);
/* g[i] = scale[0] * sign(den[i] - clean[i])  (backward of nn.L1Loss, util.py:239) */
int trunet_l1_grad(const float* den, const float* clean, const float* scale, float* g, int64_t n, void* stream);
/* out[c] = sum_g partials[g*ncols + c] in fp64 (one fp32 rounding of the sum); nparts, ncols >= 1 */
int trunet_reduce_cols(const float* partials, int nparts, int ncols, float* out, void* stream);
/* One resolution of MultiResolutionSTFTLoss (stft_loss.py:9-113): win = Hann(win_length) zero-padded to n,
 * frames = 1 + L/hop.  fwd: partials[(b*frames + f)][3] = sum (|Y|-|X|)^2, sum |Y|^2, sum |log|Y| - log|X||
 * with |.| = sqrt(clamp(re^2+im^2, 1e-7)).
 * Arguments of every STFT entry point (this one, _bwd_gather, _fwdgrad, trunet_stft_mag, trunet_stft_mag_bwd, and per
 * resolution trunet_loss_grad_gather): n a power of two, 8 <= n <= 2048 (the (2n + n/2) * 8 bytes of dynamic LDS stay
 * inside the 64 KB a kernel gets without raising its limit; n = 4096 is refused, not launched), L > n/2, hop >= 1,
 * 1 <= win_length <= n, B >= 1; anything else is TRUNET_EINVAL before a launch.
 * A frame whose windowed x and y are bit-identical has |Y| = |X| exactly (not the two results of the shared transform,
 * whose roundings differ): its first and third sums are exactly 0 and it contributes no loss gradient. */
int trunet_stft_loss_fwd(const float* x, const float* y, const float* win, const float* tw, float* partials,
                         int B, int L, int n, int hop, void* stream);
/* bwd: d loss / d x -> gx (B, L) given coef[0] = g_sc*lambda_sc/(nres*sqrt(S1)*sqrt(S2)) (0 at S1 == 0), coef[1] =
 * g_mag*lambda_mag/(nres*count).  No float atomics: the windowed frame gradients go to `frames` (B, frames, win_length:
 * the window's support, centred in n) and a gather sums them per sample; gx is written (not accumulated), deterministic. */
int trunet_stft_loss_bwd_gather(const float* x, const float* y, const float* win, const float* tw, const float* coef,
                                float* frames, float* gx, int B, int L, int n, int hop, int win_length, void* stream);
/* ---- causal audio-in -> audio-out stream (stream.py:83-109: ProcessAudio + model per chunk), S concurrent streams, one hop
 * of 128 samples per stream and call; all state lives in caller-owned device tensors with fixed addresses (hipGraph-replayable).
 * trunet_stream_features: ring (S, 512) <- [ring[:, 128:], chunk (S, 128)] (chunk NULL: the ring already holds the frame, used
 * for the reflect-padded first frame of dataset.py:260-264), then ONE frame of ProcessAudio.forward (dataset.py:246-272) per
 * stream -> feat (S, C, 257); C = 4: PCEN (dataset.py:56-76) with the smoother carried in pcen_M (S, 257) (first != 0: M = s x). */
int trunet_stream_features(float* ring, const float* chunk, float* pcen_M, float* feat, const float* tw512, int S, int C,
                           int first, float eps, float s, float alpha, float delta, float r, void* stream);
/* trunet_stream_mask_istft: net output of one frame per stream (S, 8, 257) -> phase-aware mask (phm.py:31-45) -> irFFT-512
 * (dataset.py:182-203) -> overlap-add into ola (S, 512) -> out (S, 128) = the hop that is final now / env (number of frames
 * covering it, dataset.py:293-296: torch.istft's window envelope for the rectangular window); ola shifted by one hop. */
int trunet_stream_mask_istft(const float* net_out, float* ola, float* out, const float* tw512, int S, float beta, float env,
                             void* stream);
/* ---- stream pool (streaming.StreamPool): the same two stages for sessions that start, pause and end on their own.  State
 * tensors hold one row per SLOT at fixed addresses -- ring (slots, 512), pcen_M (slots, 257), ola (slots, 512) -- and a call
 * handles the n_rows rows of one pass: row i works on slot rows[i][0].  rows: DEVICE array (n_rows, TRUNET_ROW_INTS) int32
 *   [0] slot   [1] TRUNET_ROW_* flags   [2] t: frame index   [3] a: whole hops received, this row's shift included
 *   [4] tail: the 0..127 samples after the last whole hop (closing sessions)   [5] env: frames covering the emitted hop
 *   [6] row of `chunks` (the new hop with TRUNET_ROW_SHIFT, else the tail samples when tail > 0)   [7] row of `out`, -1: none
 * A frame can be computed while a - 2 <= t <= a, and t <= 1 only while a <= 4 (what lies further back has left the ring).
 * Frame t is x[reflect(128 t + i - 256, L = 128 a + tail)], i < 512, built from the ring (x[128 a - 512, 128 a)) and the tail.
 * One real frame per workgroup: a row's results do not depend, bit for bit, on any other row of the call.  Distinct rows of
 * one call must name distinct slots.  A row whose slot is outside [0, slots), or whose chunk / feature / out row is outside
 * the given extents, is skipped without touching memory.
 * trunet_stream_features_rows: SHIFT: ring <- [ring[128:], chunks[row 6]]; unless NOFRAME: frame t -> feat[i] (C, 257) for the
 * rows i < n_frames (rows from n_frames on must be NOFRAME); C = 4: PCEN with pcen_M[slot] (FIRST: M = s x).  chunks
 * (n_chunks, 128).  A FIRST row (t = 0) transforms frames 0 and 1 of its session together, paired as the offline entry
 * points pair them, leaves frame 1's features in stash[slot] (stash: (slots, C, 257)) and the smoother after frame 1 in
 * pcen_M; the session's next row must be its frame 1 with TRUNET_ROW_STASHED, which copies them to feat[i].
 * trunet_stream_mask_istft_rows: net_out (n_rows, 8, 257) -> ola[slot] (FIRST: starts from zero) -> out[row 7] (128) = the
 * final hop / env; FINISH: out rows [7] + 1 and + 2 take the last whole hop (/ 3) and the hop of the tail samples (/ 2).
 * out (n_out, 128). */
#define TRUNET_ROW_INTS 8
#define TRUNET_ROW_SHIFT 1
#define TRUNET_ROW_FIRST 2
#define TRUNET_ROW_NOFRAME 4
#define TRUNET_ROW_FINISH 8
#define TRUNET_ROW_STASHED 16
int trunet_stream_features_rows(float* ring, const float* chunks, float* pcen_M, float* stash, float* feat,
                                const int32_t* rows, int n_rows, int n_frames, int n_chunks, int slots, const float* tw512, int C, float eps, float s,
                                float alpha, float delta, float r, void* stream);
int trunet_stream_mask_istft_rows(const float* net_out, float* ola, float* out, const int32_t* rows, int n_rows, int n_out,
                                  int slots, const float* tw512, float beta, void* stream);

/* ---- stream pool, packets of any size (StreamPool.feed): every listed session brings a packet of n >= 0 samples and all the
 * whole hops it completes are computed in the call.  Per slot the pool also keeps fifo (slots, 128): the 0..127 samples that
 * wait for their hop to fill.  A frame is a 512-sample window of its session's LINE
 *     ring[slot] (x[128 a0 - 512, 128 a0))  ++  fifo[slot][0, r0)  ++  samples[poff, poff + n)
 * with a0 whole hops and r0 pending samples before the call; samples (n_samples) holds the packets back to back.
 * rows: DEVICE array (n_rows, TRUNET_FEED_INTS) int32, record i = feature row i = net_out row i = frames row i:
 *   [0] slot   [1] TRUNET_ROW_FIRST: frame 0, computed with the session's frame 1 (one transform, as the _rows entry points
 *   pair them), whose features go to row [9]; TRUNET_ROW_STASHED: frame 1, nothing to transform   [2] t (informative)
 *   [3] offset in the line of the window's first sample (FIRST: of x[0])   [4] r0   [5] n   [6] poff
 *   [7] env: frames covering the hop this frame completes   [8] hop of `out` it goes to, -1: none   [9] FIRST: row of frame 1
 * sess: DEVICE array (n_sess, TRUNET_FEED_INTS) int32, one record per listed session:
 *   [0] slot   [1] flags (not read)   [2] seq0   [3] frames   [4] whole hops gained   [5] r0   [6] n   [7] poff
 *   [8] r1 = r0 + n - 128 [4]: pending samples after the call   [9] position in the call (informative)
 * seq: DEVICE array (n_rows) int32: seq[seq0 .. seq0 + frames) are the session's frame records in frame order.  Distinct
 * sessions of a call name distinct slots.  A record whose slot, sample range, frame list or out hop lies outside the declared
 * extents is skipped without touching state or data; every offset is an int32 and n_samples <= TRUNET_FEED_MAX_SAMPLES.
 * trunet_stream_feed_features: per frame record, the features of ProcessAudio.forward -> feat (n_rows, C, 257); C = 4 leaves
 *   the magnitude in channel 1.  Reads ring and fifo only.
 * trunet_stream_feed_commit: per session, PCEN over its frames in frame order with the smoother carried in pcen_M[slot]
 *   (FIRST: M = s x) replacing the magnitudes in feat; then ring[slot] <- line[128 [4], 128 [4] + 512) and fifo[slot] <- the
 *   r1 samples after it.  n_rows may be 0 (sessions that only store samples).  Must follow trunet_stream_feed_features.
 * trunet_stream_feed_mask_istft: net_out (n_rows, 8, 257) -> mask -> irFFT-512, unnormalised -> frames (n_rows, 512).
 * trunet_stream_feed_ola: per session (the first n_sess records of sess: those with frames), its frames onto ola[slot]
 *   (FIRST: the tail starts from zero) in frame order; after each frame out[hop [8]] (128) = the completed hop / env and
 *   the tail moves on by a hop.  out (n_out, 128); n_out may be 0. */
#define TRUNET_FEED_INTS 10
#define TRUNET_FEED_MAX_SAMPLES 0x7fff0000
int trunet_stream_feed_features(const float* ring, const float* fifo, const float* samples, float* feat, const int32_t* rows,
                                int n_rows, int n_samples, int slots, const float* tw512, int C, void* stream);
int trunet_stream_feed_commit(float* ring, float* fifo, const float* samples, float* pcen_M, float* feat, const int32_t* rows,
                              const int32_t* sess, const int32_t* seq, int n_sess, int n_rows, int n_samples, int slots, int C,
                              float eps, float s, float alpha, float delta, float r, void* stream);
int trunet_stream_feed_mask_istft(const float* net_out, float* frames, int n_rows, const float* tw512, float beta, void* stream);
int trunet_stream_feed_ola(const float* frames, float* ola, float* out, const int32_t* rows, const int32_t* sess,
                           const int32_t* seq, int n_sess, int n_rows, int n_out, int slots, void* stream);

/* ---- the attenuation limit (atten.py): out[n] = y[n] + g (x[n] - y[n]) at 16 kHz, directly behind the
 * overlap-add; y the enhanced sample a route returns, x the dry input sample at the same position, g = 10^(-L / 20) in [0, 1]
 * (g = 0: out = y bit for bit).  fp32: one subtraction and one fused multiply-add (atten_blend.hpp, shared by all three).
 * trunet_atten_blend_ragged (enhance): in place on audio (total_samples), the packed iSTFT output; dry: the packed input;
 *   gains (B): one per utterance; sample_off as in the ragged entry points above.  One launch.
 * trunet_atten_blend_rows (AudioStream): in place on out[r * out_stride + i], i < n, with dry[r * dry_stride + i] and
 *   gains[r], r < rows.  One launch.
 * trunet_stream_atten (StreamPool): per slot dry_line (slots, TRUNET_ATT_DRY_LINE) the samples at 16 kHz fed and not yet
 *   returned (at most 511), g_cur (slots) the gain the slot's session last emitted with, g_tgt (slots) the gain it is to have
 *   (written by the host only).  packet (n_packet): the call's new samples back to back; out (n_out): the call's output.
 *   plan: DEVICE array (n_sess, TRUNET_ATT_INTS) int32, one record per listed session, distinct slots:
 *     [0] slot   [1] c0: samples in its dry line   [2] offset and [3] length n of its packet   [4] offset and [5] length m of
 *     its outputs in out (m <= c0 + n)   [6] TRUNET_ATT_FIRST: the call holds frame 0 of the session, which starts at its
 *     target (g_cur is not read); TRUNET_ATT_CLOSING: the session ends, m = c0 + n and nothing is kept   [7] zero.
 *   A workgroup per record: with line = [dry_line[slot][0, c0) | packet[[2], [2] + n)], out[[4] + k] = blend(out[[4] + k],
 *   line[k], g_k), k < m, where g_k = g_tgt[slot], except over k < 128 when g_cur differs from it: g_k = g_cur + (g_tgt -
 *   g_cur) (k + 1) / 128, g_127 = g_tgt -- the first hop a session emits after a change.  Then dry_line[slot] <- line[m, c0 +
 *   n) and, when FIRST or m > 0, g_cur[slot] <- g_tgt[slot].  One launch, after the overlap-add on the same stream.
 * TRUNET_EINVAL without a launch for anything the host can see; a record whose slot, packet, outputs or remainder lie outside
 * slots, n_packet, n_out or the line is skipped before any load or store. */
#define TRUNET_ATT_INTS 8
#define TRUNET_ATT_DRY_LINE 512
#define TRUNET_ATT_FIRST 1
#define TRUNET_ATT_CLOSING 2
int trunet_atten_blend_ragged(float* audio, const float* dry, const float* gains, const int64_t* sample_off, int B,
                              int64_t total_samples, void* stream);
int trunet_atten_blend_rows(float* out, const float* dry, const float* gains, int rows, int n, int out_stride, int dry_stride,
                            void* stream);
int trunet_stream_atten(float* out, float* dry_line, float* g_cur, const float* g_tgt, const float* packet,
                        const int32_t* plan, int n_sess, int slots, int n_packet, int n_out, void* stream);

/* ---- offline enhancement of B utterances of any lengths (enhance.py), packed back to back ----
 * audio holds sum L_b samples (L_b >= 257); sample_off[B+1] (prefix of L_b), frame_off[B+1] (prefix of T_b = 1 + L_b/128)
 * and pair_off[B+1] (prefix of ceil(T_b/2)) are int64 DEVICE arrays; total_* are their last entries.  Frames are paired
 * per utterance exactly as the dense entry points pair them, so every utterance's result is bit for bit the dense entry
 * point's on that utterance alone.  An utterance whose offsets are inconsistent or leave the declared totals is skipped.
 * trunet_stft_features_ragged: trunet_stft_features per utterance -> feat (sum T, C, 257), mag (sum T, 257) if non-NULL.
 * trunet_pcen_ragged: trunet_pcen with the smoother restarted at each utterance's first frame.
 * trunet_mask_istft_ragged: trunet_mask_istft_fwd per utterance without the L1 sums -> audio (sum L) with all L_b samples
 * of each utterance (torch.istft(..., length = L_b)); frames: scratch (sum T, 512). */
int trunet_stft_features_ragged(const float* audio, const int64_t* sample_off, const int64_t* frame_off,
                                const int64_t* pair_off, float* feat, float* mag, const float* tw512, int B,
                                int64_t total_samples, int64_t total_frames, int64_t total_pairs, int C, void* stream);
int trunet_pcen_ragged(const float* mag, float* out, const int64_t* frame_off, int B, int64_t total_frames, int out_stride,
                       float eps, float s, float alpha, float delta, float r, void* stream);
int trunet_mask_istft_ragged(const float* net_out, float* frames, float* audio, const int64_t* sample_off,
                             const int64_t* frame_off, const int64_t* pair_off, const float* tw512, int B,
                             int64_t total_samples, int64_t total_frames, int64_t total_pairs, float beta, void* stream);

/* ---- speech-quality metrics of B clean / estimate pairs of any lengths (evaluate.py), packed back to back ----
 * Offsets are int64 DEVICE prefix arrays of B+1 entries, total_* their last entries; an utterance whose offsets are
 * inconsistent with each other or leave the totals is skipped.  No call reads anything back to the host: every buffer is
 * sized by counts the host knows from the lengths.  Each utterance's results are bit for bit independent of its batch-mates.
 * trunet_resample_ragged: nsig (1 or 2) planes of total_in samples -> planes of total_out; out_off = prefix of
 *   ceil(L_b p / q); y[m] = p sum_n taps[m q - n p + half] x[n] over the 2*half+1 taps (scipy.signal.resample_poly with
 *   that window); p, q <= 64, half <= 4096.
 * trunet_stoi_ragged: STOI and ESTOI (fp64) and the segment count (int64) per utterance of sig = (2, total_samples), clean
 *   then estimate at 10 kHz.  sig_off: prefix of R_b; frame_off: of F_b = |range(0, R_b - 256, 128)|; seg_off: of
 *   max(F_b - 30, 0); chunk_off: of ceil(max(F_b - 30, 0) / 64).  window: 256 floats, band_edges: 16 ints (band k = bins
 *   [e[k], e[k+1]) of the 512-point FFT), workspace: trunet_stoi_workspace_bytes(B, total_frames, total_segments) bytes.
 * trunet_si_sdr_ragged: SI-SDR in dB (fp64) per utterance; chunk_off: prefix of ceil(L_b / 16384); partials: 5 doubles per
 *   chunk. */
int trunet_resample_ragged(const float* in, float* out, const int64_t* in_off, const int64_t* out_off, const float* taps,
                           int half, int p, int q, int B, int64_t total_in, int64_t total_out, int nsig, void* stream);
/* trunet_resample_rational (resample.py): the same definition and the same in_off / out_off tables for any
 * ratio with p, q <= 640, total_in and total_out below 2^31.  A workgroup stages the input span of one tile of `tile`
 * consecutive outputs of one utterance (tiles counted from the utterance's first output; tile a multiple of 256, at most
 * 4096) in LDS; tile_off = int64 DEVICE prefix of ceil(M_b / tile), M_b = ceil(L_b p / q), total_tiles its last entry.
 * half = zeros * max(p, q) with 1 <= zeros <= 32, K = ceil((2 half + 1) / p); table = the taps phase-major, p rows of
 * Kp = K rounded up to a multiple of 4 floats, table[r * Kp + k] = taps[r + k p] (zero past the last tap), 16-byte aligned.
 * taps_in_lds: 1 = every workgroup copies the table into LDS (p * Kp <= 16384), 0 = rows are read from L2.  fp32
 * accumulation per output with k ascending; results are bit for bit independent of the batch.  TRUNET_EINVAL without a
 * launch for anything the host can see; an utterance whose device offsets contradict each other is skipped. */
int trunet_resample_rational(const float* in, float* out, const int64_t* in_off, const int64_t* out_off,
                             const int64_t* tile_off, const float* table, int half, int K, int p, int q, int tile, int B,
                             int64_t total_in, int64_t total_out, int64_t total_tiles, int nsig, int taps_in_lds,
                             void* stream);
/* trunet_resample_stream / trunet_resample_stream_commit (resample.py: StreamResampler): the same
 * definition, taps table and per-output expression for sessions that arrive in packets; the outputs of a session, however it
 * is cut, are bit for bit those of trunet_resample_rational on the whole.  hist (slots, K - 1): per slot the last K - 1
 * samples of its session (K - 1 <= TRUNET_RS_STREAM_MAX_HISTORY); in (n_in): the packets of the call back to back; out
 * (n_out); plan: DEVICE array (n_sess, TRUNET_RS_STREAM_INTS) int64, one record per listed session, distinct slots:
 *   [0] slot   [1] N0: samples the session had before the call   [2] offset and [3] length n >= 0 of its packet in `in`
 *   [4] m0: its first output of the call   [5] outputs   [6] their offset in `out`   [7] closing: outputs up to
 *   ceil((N0 + n) p / q) with zeros right of the session, and no history is kept   [8], [9] its tiles [t0, t1) of the grid,
 *   t1 - t0 = ceil(outputs / tile); n_tiles = the last t1.
 * An open session owes the outputs below max(0, ceil(((N0 + n) p - half) / q)): they read no sample at or past N0 + n, and
 * the next one reads none below N0 + n - (K - 1).  trunet_resample_stream: a workgroup per tile, reads hist only.
 * trunet_resample_stream_commit, after it on the same stream: a workgroup per session, hist[slot] <- the last K - 1 samples
 * of [hist[slot] | packet] (zeros left of sample 0).  TRUNET_EINVAL without a launch for anything the host can see; a record
 * whose slot, packet, outputs or tiles lie outside slots, n_in, n_out or n_tiles is skipped by both kernels.
 * All three entry points are resample.hip, and both tile kernels run its one tile function; resample.py lays its calls out
 * by the limits below (tests/test_resample_cpu.py compares the two). */
#define TRUNET_RS_MAX_TILE 4096             /* outputs per workgroup, at most */
#define TRUNET_RS_SPAN_MAX 4608             /* floats of input a workgroup stages per window */
#define TRUNET_RS_TAPS_LDS_MAX 16384        /* floats of the tap table that may live in LDS */
#define TRUNET_RS_STREAM_INTS 10
#define TRUNET_RS_STREAM_MAX_HISTORY 20480
int trunet_resample_stream(const float* hist, const float* in, float* out, const int64_t* plan, const float* table, int half,
                           int K, int p, int q, int tile, int n_sess, int slots, int64_t n_in, int64_t n_out, int64_t n_tiles,
                           int taps_in_lds, void* stream);
int trunet_resample_stream_commit(float* hist, const float* in, const int64_t* plan, int half, int K, int p, int q, int n_sess,
                                  int slots, int64_t n_in, void* stream);
/* trunet_highband_gains / trunet_highband_join (highband.py): the band above 8 kHz of audio at fs > 16 kHz
 * around the 16 kHz enhancement.  lo, y16 (total_samples each): the utterances at 16 kHz before and after the enhancement,
 * packed back to back; sample_off, frame_off: int64 DEVICE prefixes of L_b and of T_b = 1 + L_b / 128; hp: the
 * TRUNET_HB_TAPS taps of the zero-phase high-pass; energy: scratch of 2 total_frames floats.
 * trunet_highband_gains: g (total_frames), g[t] = clamp(sqrt((e_y + 1e-10) / (e_x + 1e-10)), g_min, 1) with e_x, e_y the
 *   energies of hp * lo and hp * y16 ("same", zeros outside the utterance) over [128 t - 256, 128 t + 256) n [0, L_b);
 *   0 < g_min <= 1.  Two launches (hop-block energies, then the frames); every sum runs in a fixed order, no atomics.
 * trunet_highband_join: out[n] = up_y[n] + G[n] (x[n] - up_x[n]) per utterance, n < L_b.  x, out (total_samples at fs) are
 *   packed by sample_off; up_y, up_x (total_up each) by up_off, utterance b having at least L_b samples there; pd / qd =
 *   16000 / fs in lowest terms, pd < qd <= 640.  TRUNET_HB_KEEP: G = 1, g and frame_off may be NULL.  TRUNET_HB_FOLLOW:
 *   G[n] = (1 - a) g[t0] + a g[min(t0 + 1, T_b - 1)], t0 = n pd / (128 qd), a = (n pd % (128 qd)) / (128 qd), with g and
 *   frame_off as trunet_highband_gains leaves them for L16_b = ceil(L_b pd / qd).
 * Totals below 2^31.  TRUNET_EINVAL without a launch for anything the host can see; an utterance whose device offsets
 * contradict each other is skipped.  Results are bit for bit independent of the batch. */
#define TRUNET_HB_TAPS 63
#define TRUNET_HB_RUN 16                    /* hop blocks of one utterance a workgroup of the energy kernel owns */
#define TRUNET_HB_JOIN_TILE 4096            /* samples of one utterance a workgroup of the join owns */
#define TRUNET_HB_KEEP 1
#define TRUNET_HB_FOLLOW 2
int trunet_highband_gains(const float* lo, const float* y16, const int64_t* sample_off, const int64_t* frame_off,
                          const float* hp, float* energy, float* g, int B, int64_t total_samples, int64_t total_frames,
                          float g_min, void* stream);
int trunet_highband_join(const float* up_y, const float* up_x, const float* x, const float* g, float* out,
                         const int64_t* sample_off, const int64_t* up_off, const int64_t* frame_off, int B,
                         int64_t total_samples, int64_t total_up, int64_t total_frames, int pd, int qd, int mode,
                         void* stream);
/* trunet_stream_highband_* (stream_highband.py, StreamPool(highband=)): the same band for sessions that
 * arrive in packets.  Per slot: x_line (slots, xcap) the samples at fs fed and not yet returned; lo_line (slots,
 * TRUNET_SHB_LO_LINE) the samples of lo whose ys16 has not come back; "follow" only: halo (slots, 62, 2) the last 62 samples
 * of lo and ys16 interleaved, estate (slots, 3, 2) the last three block energies (E_x, E_y), gstate (slots, 2) the last two
 * block gains.  Per call: packet (n_packet) the packets at fs and x16 (n_x16) their down-resampled samples, back to back;
 * paired, ys16 (n_paired): the lo that pairs with the call's ys16, and that ys16; up_y, up_x, out (n_up); eline (n_blocks +
 * 3 n_sess, 2) and gline (n_blocks + 2 n_sess): per record the slot's last three energies / two gains, then the call's new
 * blocks.  plan: DEVICE array (n_sess, TRUNET_SHB_INTS) int64, one record per listed session, distinct slots:
 *   [0] slot   [1] samples in its x line   [2] offset and [3] length of its packet   [4] offset of its outputs in up_y, up_x
 *   and out   [5] outputs to write (<= [1] + [3])   [6] samples in its lo line   [7] offset and [8] length of its new x16
 *   [9] offset and [10] length pn of its paired samples (<= [6] + [8])   [11] outputs it was given before the call
 *   [12] hop blocks complete before the call   [13] new blocks bn: pn / 128, or ceil(pn / 128) when closing   [14] its first
 *   tile of the join (TRUNET_SHB_TILE outputs each)   [15] closing: nothing of the slot is kept   [16] its first tile of the
 *   pairing   [17] the sum of [13] over the records before it.
 * pair: paired <- the first pn samples of [lo line | x16].  gains: eline, then gline (two launches).  join: out[n] =
 * up_y[n] + G[n] (x[n] - up_x[n]) with x from [x line | packet]; TRUNET_HB_KEEP: G = 1 and gline may be NULL;
 * TRUNET_HB_FOLLOW: G[n] = ((D - c) g_c[max(j - 1, 0)] + c g_c[j]) / D, s = ([11] + n) pd, D = 128 qd, j = s / D, c = s % D.
 * commit, after them on the same stream: the lines drop what was consumed and take what came, and the "follow" state moves
 * on.  pair, gains and join only read the per-slot state.  TRUNET_EINVAL without a launch for anything the host can see; a
 * record that leaves the extents passed in is skipped by every kernel. */
#define TRUNET_SHB_INTS 18
#define TRUNET_SHB_LO_LINE 512
#define TRUNET_SHB_MAX_X_LINE 4096
#define TRUNET_SHB_TILE 1024
int trunet_stream_highband_pair(const float* lo_line, const float* x16, float* paired, const int64_t* plan, int n_sess,
                                int slots, int xcap, int64_t n_packet, int64_t n_up, int64_t n_x16, int64_t n_paired,
                                int64_t n_blocks, int64_t n_tiles, void* stream);
int trunet_stream_highband_gains(const float* paired, const float* ys16, const float* halo, const float* estate,
                                 const float* gstate, const float* hp, float* eline, float* gline, const int64_t* plan,
                                 int n_sess, int slots, int xcap, int64_t n_packet, int64_t n_up, int64_t n_x16,
                                 int64_t n_paired, int64_t n_blocks, float g_min, void* stream);
int trunet_stream_highband_join(const float* up_y, const float* up_x, const float* x_line, const float* packet,
                                const float* gline, float* out, const int64_t* plan, int n_sess, int slots, int xcap,
                                int64_t n_packet, int64_t n_up, int64_t n_x16, int64_t n_paired, int64_t n_blocks,
                                int64_t n_tiles, int pd, int qd, int mode, void* stream);
int trunet_stream_highband_commit(float* x_line, const float* packet, float* lo_line, const float* x16, float* halo,
                                  const float* paired, const float* ys16, float* estate, const float* eline, float* gstate,
                                  const float* gline, const int64_t* plan, int n_sess, int slots, int xcap, int64_t n_packet,
                                  int64_t n_up, int64_t n_x16, int64_t n_paired, int64_t n_blocks, int mode, void* stream);
size_t trunet_stoi_workspace_bytes(int B, int64_t total_frames, int64_t total_segments);
int trunet_stoi_ragged(const float* sig, const int64_t* sig_off, const int64_t* frame_off, const int64_t* seg_off,
                       const int64_t* chunk_off, const float* window, const int* band_edges, const float* tw512,
                       void* workspace, double* stoi, double* estoi, int64_t* segments, int B, int64_t total_samples,
                       int64_t total_frames, int64_t total_segments, int64_t total_chunks, void* stream);
int trunet_si_sdr_ragged(const float* clean, const float* estimate, const int64_t* sample_off, const int64_t* chunk_off,
                         double* partials, double* out, int B, int64_t total_samples, int64_t total_chunks, void* stream);
/* The intelligibility loss -(lambda / B) sum_b s_b, s_b the STOI (extended = 0) or ESTOI (1) above (stoi_loss.py, DESIGN
 * section 3q).  Its forward is trunet_stoi_ragged; the backward reads that call's inputs and its workspace (kept frames,
 * counts, band magnitudes), all of the clean signal being a constant.
 * trunet_stoi_loss_bwd: grad (total_samples) = d loss / d estimate at 10 kHz, with scale = -lambda / B and gout the (1,)
 *   DEVICE cotangent of the loss; an utterance without a segment gets exact zeros.  bwd_workspace:
 *   trunet_stoi_loss_workspace_bytes(B, total_frames, total_segments) bytes.  Four launches (segments, frame gather, bands,
 *   samples), no atomics: an utterance's gradient is bit for bit independent of its batch-mates.
 * trunet_resample_ragged_bwd: the adjoint of trunet_resample_ragged for one plane: gin (total_in) from gout (total_out).
 * trunet_stoi_loss_value: out[0] = (float)(-mean_b scores[b]) (fp64, b ascending), out[1] = lambda * out[0];
 *   loss_accum (may be NULL): loss_accum[0] += out[1]. */
size_t trunet_stoi_loss_workspace_bytes(int B, int64_t total_frames, int64_t total_segments);
int trunet_stoi_loss_bwd(const float* sig, const int64_t* sig_off, const int64_t* frame_off, const int64_t* seg_off,
                         const int64_t* chunk_off, const float* window, const int* band_edges, const float* tw512,
                         const void* fwd_workspace, void* bwd_workspace, const float* gout, double scale, int extended,
                         float* grad, int B, int64_t total_samples, int64_t total_frames, int64_t total_segments,
                         int64_t total_chunks, void* stream);
int trunet_resample_ragged_bwd(const float* gout, float* gin, const int64_t* in_off, const int64_t* out_off,
                               const float* taps, int half, int p, int q, int B, int64_t total_in, int64_t total_out,
                               void* stream);
int trunet_stoi_loss_value(const double* scores, int B, float lambda, float* out, float* loss_accum, void* stream);

/* ---- the train step's loss as util.loss_fn composes it (util.py:239-250, stft_loss.py:141-166), fused (round 4) ----
 * trunet_stft_loss_fwdgrad: trunet_stft_loss_fwd's three sums per frame AND the two coefficient-free gradient frames of the
 * same resolution (fr_sc, fr_mag: (B, frames, win_length)) from one pass: the gradient of a resolution is
 * c_sc * OLA(fr_sc) + c_mag * OLA(fr_mag) with coefficients known only after the grid-wide sums. */
int trunet_stft_loss_fwdgrad(const float* x, const float* y, const float* win, const float* tw, float* partials,
                             float* fr_sc, float* fr_mag, int B, int L, int n, int hop, int win_length, void* stream);
#define TRUNET_MAX_RES 8
typedef struct trunet_loss_args {
    const float* l1_partials;              /* trunet_mask_istft_fwd's per-block sums of |audio - clean| */
    const float* parts[TRUNET_MAX_RES];    /* per resolution: (nrows, 3) sums of trunet_stft_loss_fwd(grad) */
    int32_t n_l1, nres;
    int32_t nrows[TRUNET_MAX_RES];         /* B * frames */
    double l1_count;                       /* B * L */
    double count[TRUNET_MAX_RES];          /* B * frames * (n/2 + 1) */
    float sc_lambda, mag_lambda, stft_lambda, _pad;
} trunet_loss_args;
/* One launch: every column sum in fp64 and the scalar algebra of util.py:239-250 / stft_loss.py:151-166:
 * loss_out[0] = l1 + stft_lambda * (sc_lambda * sum_i sqrt(S1_i)/sqrt(S2_i) + mag_lambda * sum_i S3_i/count_i) / nres;
 * vals (>= 5 + 2 nres floats): [0] loss [1] l1 [2] stft_sc term [3] stft_mag term [4] 1/(B L) [5+2i] c_sc_i [6+2i] c_mag_i
 * (the backward coefficients for an upstream gradient of 1); c_sc_i is 0 where S1_i == 0 (x equals y in every bin: the
 * gradient of sqrt(S1)/sqrt(S2) is 0 there, as torch's norm has it, not the inf of 1/(sqrt(S1) sqrt(S2))).
 * scratch: trunet_loss_scratch_bytes() bytes, ZERO on first use (the kernel leaves ALL of it zero).
 * Arguments: n_l1 >= 1, l1_count > 0, 0 <= nres <= TRUNET_MAX_RES, per resolution nrows >= 1 and count > 0 (a NaN count
 * is refused); anything else is TRUNET_EINVAL before a launch. */
size_t trunet_loss_scratch_bytes(void);
int trunet_loss_finalize(const trunet_loss_args* a, float* loss_out, float* vals, void* scratch, void* stream);
typedef struct trunet_loss_gather_args {
    const float* fr_sc[TRUNET_MAX_RES];
    const float* fr_mag[TRUNET_MAX_RES];
    int32_t n[TRUNET_MAX_RES], hop[TRUNET_MAX_RES], win_length[TRUNET_MAX_RES];
    int32_t nres, _pad;
} trunet_loss_gather_args;
/* d loss / d audio (B, L) in one deterministic gather: g_loss[0] * (vals[4] * sign(audio - clean) + sum_i (vals[5+2i] *
 * OLA_i(fr_sc_i) + vals[6+2i] * OLA_i(fr_mag_i))) -- autograd of nn.L1Loss (util.py:239) + stft_loss.py:9-113.
 * sign(0) = 0; 0 <= nres <= TRUNET_MAX_RES, B, L >= 1, and per resolution the STFT argument ranges above. */
int trunet_loss_grad_gather(const trunet_loss_gather_args* a, const float* audio, const float* clean, const float* vals,
                            const float* g_loss, float* g_audio, int B, int L, void* stream);
/* stft() of stft_loss.py:9-30: magnitudes sqrt(clamp(re^2+im^2, 1e-7)) of the Hann-windowed, centre/reflect-padded STFT
 * as (B, 1 + L/hop, n/2 + 1); y / ymag may be NULL (one signal), else both signals share one complex FFT. */
int trunet_stft_mag(const float* x, const float* y, const float* win, const float* tw, float* xmag, float* ymag, int B,
                    int L, int n, int hop, void* stream);
/* backward of trunet_stft_mag for x (autograd of stft_loss.py:9-30): gmag (B, frames, n/2+1) = cotangent of the
 * magnitudes -> gx (B, L); frames: scratch (B, frames, win_length); same recompute + gather scheme as above. */
int trunet_stft_mag_bwd(const float* x, const float* win, const float* tw, const float* gmag, float* frames, float* gx,
                        int B, int L, int n, int hop, int win_length, void* stream);
/* PhaseAwareMask.forward (phm.py:31-45 + R5) on interleaved complex64: out = sigmoid(beta(angle m - angle e)) |m| */
int trunet_phm_fwd(const float* mix_ri, const float* est_ri, float* out, int64_t n, float beta, void* stream);
/* its backward (autograd of phm.py:31-45): g_out real (n) -> gradients of the two complex inputs in torch's convention
 * (d/d re + j d/d im, interleaved); either output may be NULL */
int trunet_phm_bwd(const float* mix_ri, const float* est_ri, const float* g_out, float* g_mix_ri, float* g_est_ri,
                   int64_t n, float beta, void* stream);

/* ---- eval-mode single-launch forward (SURVEY 8f ranks 1 + 2; rt.py:20-27 protocol, onnx.py:14-44 artefact role) ----
 * The whole TRU-Net forward of network.py:153-171 (R1-R4) for N frames in ONE launch: x (N, Cin, 257) -> y (N, 8, 257),
 * Cin in {3, 4}.  BatchNorm (eval: running statistics) is folded into the conv in front of it by the exporter; `blob` is
 * the exported weight image of `blob_numel` floats (32-row tiles for the 128-channel encoder layers, 16-row tiles for the
 * GRU projection and every 64-channel layer, each in MFMA fragment order) and h_offsets the 30 element offsets of its
 * sections (first conv | 5 encoder pw | 5 depthwise | GRU projection | W_hh, b_hh | FGRU conv | 6 decoder pw | 5 transposed
 * convs | last transposed conv | TGRU r/z rows, n rows of W_ih, n rows of W_hh, TGRU conv -- the last four 0 when the
 * time-recurrent block was not exported), as written by tinyrecurrentunet_amd/export.py.  Every workgroup takes one frame
 * at a time through all layers in its own LDS; `scratch` holds the skip tensors of the frames in flight:
 * trunet_stream_fwd_scratch_floats(trunet_stream_fwd_grid(N)) floats.
 * h_in == h_out == NULL: every frame independent (the reference's forward, TGRU not executed, R4).
 * h_in, h_out != NULL (the causal stream of rt.py:20-27 / stream.py:83-109; network.py:150, GRUBlock :45-58): the N frames
 * are ONE new frame of N streams; the TGRU block runs one GRU time step per (stream, frequency position) between
 * FGRU.conv and decoder.0; h_in / h_out are (N, 128, 16) fp32 hidden states (may be the same buffer: updated in place).
 * trunet_stream_fwd_check: TRUNET_OK when every section (fragment over-reads included) lies inside the blob; the launch
 * entry point runs it first, so a truncated or foreign image returns TRUNET_EINVAL instead of faulting. */
int trunet_stream_fwd_grid(int N);
size_t trunet_stream_fwd_scratch_floats(int grid);
int trunet_stream_fwd_check(const int32_t* h_offsets, int n_offsets, int64_t blob_numel, int Cin);
int trunet_stream_fwd(const float* x, float* y, const float* blob, const int32_t* h_offsets, int n_offsets,
                      int64_t blob_numel, float* scratch, const float* h_in, float* h_out, int N, int Cin, void* stream);
/* The same forward with the matrix layers of SFX_MASK (stream_fwd.hip) on the bf16 MFMA through the three-term split of the fp32
 * operands (fp32-grade result: section 3b of DESIGN.md): identical contract, but `blob` is the image export.x3_image() derives
 * from the folded one -- those layers' weights as three bf16 fragment planes (an exact split of the folded fp32 weights), every
 * other section bit for bit -- passed as 32-bit words; trunet_stream_fwd_x3_check is its bounds check. */
int trunet_stream_fwd_x3_mask(void);     /* layer groups on the split path in this build (export._X3_SECTIONS) */
int trunet_stream_fwd_x3_check(const int32_t* h_offsets, int n_offsets, int64_t blob_numel, int Cin);
int trunet_stream_fwd_x3(const float* x, float* y, const float* blob, const int32_t* h_offsets, int n_offsets,
                         int64_t blob_numel, float* scratch, const float* h_in, float* h_out, int N, int Cin, void* stream);
/* The stateless forward on the int8 MFMA (stream_fwd_i8.hip): `blob` is the quantized image of
 * tinyrecurrentunet_amd/quantize.py, `blob_bytes` long (a multiple of 4), h_offsets its 26 section offsets in 32-bit words
 * (the 26 sections of trunet_stream_fwd: the matrix layers and W_hh as int8 with per-row fp32 scales, the first conv, the
 * depthwise convs and the last transposed conv fp32).  Activations are quantized per frame and per layer, so every frame is
 * independent of its batch-mates.  Same grid and scratch as trunet_stream_fwd; the kernel re-checks the offsets.
 * trunet_i8_mfma_probe: one 16 x 64 (int8, row-major) by 64 x 16 product through the lane maps the kernel uses -> 16 x 16
 * int32, for the tests. */
int trunet_stream_fwd_i8_check(const int32_t* h_offsets, int n_offsets, int64_t blob_bytes, int Cin);
int trunet_stream_fwd_i8(const float* x, float* y, const void* blob, const int32_t* h_offsets, int n_offsets,
                         int64_t blob_bytes, float* scratch, int N, int Cin, void* stream);
int trunet_i8_mfma_probe(const void* a, const void* b, int* c, void* stream);

/* ---- input pipeline on the GPU ----
 * DataAugment.__call__ + the clean/noise mix (dataset.py:116-126, :380) for a whole batch resident in HBM:
 *   noise' = clamp(hp(clamp(lp(gain * noise), -1, 1)), -1, 1);   noisy = clean + noise'      (clean == NULL: noisy = noise')
 * noise, clean, noisy, noise_out (optional copy of noise') are (B, L); params is (B, 11) = linear gain, then the low-pass
 * and the high-pass biquad as b0, b1, b2, a1, a2 (normalised by a0; torchaudio.functional.lowpass_biquad /
 * highpass_biquad -> lfilter(clamp=True), the calls of dataset.py:123-125).  noisy must not alias noise. */
int trunet_augment_mix(const float* noise, const float* clean, const float* params, float* noisy, float* noise_out, int B,
                       int L, void* stream);

/* ---- reverberant training pairs (build extension: the reference has gain and biquads only) ----
 * Per row b of (B, L) signals, with h = rir[b][0 .. K_b), K_b = clamp(rir_len[b], 0, Kmax), h[0] the direct path:
 *   wet[n]  = sum_{k < K_b, k <= n} h[k] clean[n-k]                  (causal, truncated to L)
 *   target  = clean when early_taps == 0, else the same sum over k < min(early_taps, K_b)   (dereverberation target)
 *   g       = sqrt(Ps / (Pv 10^(snr_db[b]/10))), Ps = mean(wet^2), Pv = mean(noise^2); g = 1 when snr_db == NULL or when
 *             Ps or Pv < 1e-20
 *   noisy   = wet + g noise;  m = max|noisy| > peak > 0  =>  noisy and target are both multiplied by peak / m
 * A row with K_b == 0 does not reverberate: wet = target = clean bit for bit (not through the transform).  rir == NULL: no
 * row reverberates (rir_len, ws and Kmax are then unused; Kmax may be 0).  noise is the ALREADY augmented noise (what
 * trunet_augment_mix writes to noise_out, or to noisy when it is given no clean signal) or NULL; rir is (B, Kmax) with taps at or beyond K_b padding that is never read as data; rir_len
 * and snr_db are (B) on the device, so a call needs no device -> host copy.  Uniformly partitioned overlap-save convolution
 * (1024-tap partitions, 2048-point transforms), no atomics: bit for bit repeatable, and a row's result does not depend on
 * its batch-mates or on Kmax.  ws: trunet_reverb_workspace_bytes(B, L, Kmax) bytes, 8-byte aligned (0 for arguments out of
 * range); its content is scratch.  TRUNET_EINVAL: NULL clean / noisy / target, rir without rir_len, B, L <= 0, Kmax <= 0
 * with rir, early_taps < 0, a workspace that is missing or too small, or noisy / target / ws overlapping each other or an
 * input.  TRUNET_ENOTSUP: Kmax > 65536. */
size_t trunet_reverb_workspace_bytes(int B, int L, int Kmax);
int trunet_reverb_mix(const float* clean, const float* noise, const float* rir, const int* rir_len, const float* snr_db,
                      int early_taps, float peak, float* noisy, float* target, void* ws, size_t ws_bytes, int B, int L,
                      int Kmax, void* stream);

/* ---- room simulation: image-source RIRs with a diffuse tail (build extension) ----
 * rooms is (B, row_floats) on the device, row_floats == 18: Lx Ly Lz | sx sy sz | rx ry rz | bx0 bx1 by0 by1 bz0 bz1 | rt60 |
 * seed_lo seed_hi (metres, reflection coefficients with x0 the wall at x = 0 and x1 the wall at x = Lx, seconds, the two 16-bit
 * halves of the seed as exactly representable floats).  Per row, K_b = clamp(round(min(rt60, max_rir_sec) fs), 1, Kmax):
 *   taps [0, min(n_c, K_b))   image-source method: sum over the images I of  gain 0.5 (1 + cos(2 pi (n - tau) / tw)) sinc(n - tau),
 *                             |n - tau| < tw / 2, tau = (|I - r| - |s - r|) fs / c, gain = prod beta^order |s - r| / |I - r|:
 *                             the direct path is exactly a unit tap at n = 0
 *   taps [n_c, K_b)           sigma_c g(seed, n) exp(-6.9078 (n - n_c + W/2) / (rt60 fs)), W = max(round(0.010 fs), 1),
 *                             sigma_c^2 the mean square of the W (at most n_c) taps before n_c, g a counter-based standard normal
 *   taps [K_b, Kmax)          zeros;   rir_len[b] = K_b
 * A row that is all zero or malformed (NaN, Inf, a dimension below 2 m, source or microphone not strictly inside or closer than
 * 1 mm to each other, |beta| > 1, rt60 <= 0, seed halves that are not integers in [0, 65535]) gives rir_len[b] = 0 and a zero
 * row.  Image orders are clamped to 96 per axis, so the work of a call is bounded whatever the rows hold.  Fixed-point
 * accumulation (2^-40) in LDS, no float atomics: a row's taps repeat bit for bit, alone, in any batch and under any Kmax.
 * ws: trunet_rir_ism_workspace_bytes(B, Kmax) bytes (0 for arguments out of range), reserved.  TRUNET_EINVAL: NULL rooms / rir /
 * rir_len / ws, row_floats != 18, B outside [1, 65535], Kmax, n_c or tw < 1, fs, c or max_rir_sec not positive and finite, a
 * short workspace.  TRUNET_ENOTSUP: Kmax > 65536, n_c > 8192, tw even or above 129, (n_c + tw/2 + 1) c / fs > 360 m. */
size_t trunet_rir_ism_workspace_bytes(int B, int Kmax);
int trunet_rir_ism(const float* rooms, int row_floats, float* rir, int32_t* rir_len, int B, int Kmax, float fs, float c,
                   int n_c, int tw, float max_rir_sec, void* ws, size_t ws_bytes, void* stream);

/* ---- time-domain loss terms: segmental cosine similarity (cos_loss.py:4-56 repaired, R8) and SI-SDR ----
 * x = audio (the estimate), y = clean, both (B, L) fp32.
 * Cosine term: bounds[0 .. nseg] = 0, g[0], g[1], ... each clipped to L gives the nseg segments [bounds[i], bounds[i+1]):
 *   cos_{b,i} = <x,y> / (c_x c_y),  c_x = max(|x|, cos_eps), c_y = max(|y|, cos_eps)  over the segment (the clamp of
 *   torch.nn.CosineSimilarity: per norm); an empty segment has cos = 0 and no gradient;
 *   L_cos = (1/nseg) sum_i mean_b (1 - cos_{b,i});
 *   d L_cos / d x = w (a_y y + a_x x) on the segment, w = 1/(nseg B), a_y = -1/(c_x c_y),
 *   a_x = <x,y> / (c_x^2 c_y |x|) when |x| > cos_eps, else 0; samples outside every segment get no gradient.
 * SI-SDR term, per row over all L samples, both signals zero-mean (Sxy, Sxx, Syy the centred sums, d = si_sdr_eps):
 *   alpha = Sxy/Syy, P = Sxy^2/Syy, N = Sxx - P, sisdr_b = 10 log10((P + d)/(N + d)), L_sisdr = -mean_b sisdr_b;
 *   d sisdr_b / d x = c_y (y - mean y) + c_x (x - mean x), c_y = k (2 alpha/(P + d) + 2 alpha/(N + d)), c_x = -2k/(N + d),
 *   k = 10/ln 10; a row with Syy == 0 contributes 0 and gets no gradient (the mean still divides by B).
 * Work is split into items (segment, piece): piece k of segment i covers samples [s_i + k P, min(s_i + (k+1) P, e_i)),
 * P = TRUNET_WAVE_LOSS_PIECE; segment nseg is the SI-SDR pseudo-segment [0, L).  The caller lists the items in the DEVICE
 * table `items` (n_items, 2) = (segment, piece), segment by segment with pieces ascending, and seg_first (nseg + 2) holds
 * the index of each segment's first item (seg_first[nseg + 1] = n_items).  A term without items is not computed: no
 * SI-SDR items -> sisdr terms and coefficients are 0; nseg = 0 -> no cosine term.  A segment whose bounds are not
 * increasing or leave [0, L], or whose item list is not exactly its pieces, is skipped: term 0, no gradient.
 * trunet_wave_loss_fwd (2 launches): fp64 partial sums per item and row into ws, then one launch that writes
 *   terms (B, nseg + 1): 1 - cos_{b,i} per segment, then sisdr_b;
 *   coef (B, nseg + 1, 3) = (A, B_, C) with  d (weighted sum) / d x = A y + B_ x + C  on the segment (w, the lambdas and
 *     the means included);
 *   vals (5): [0] cos_lambda L_cos + si_sdr_lambda L_sisdr  [1] L_cos  [2] mean_b sisdr_b (dB)  [3] cos_lambda L_cos
 *     [4] si_sdr_lambda L_sisdr;   loss_accum (may be NULL): loss_accum[0] += vals[0].
 *   All of it fp64, rounded once on store.  No atomics: bit for bit repeatable; a row's terms and coefficients do not depend
 *   on its batch-mates.  ws: trunet_wave_loss_workspace_bytes(B, L, nseg) bytes, 8-byte aligned (0 for extents out of range).
 * trunet_wave_loss_grad (1 launch): g_audio[b][i] += g_loss[0] * sum over the segments containing i of (A y + B_ x + C).
 * TRUNET_EINVAL before any launch: NULL buffers (loss_accum excepted), B outside [1, 65535], L outside [1, 2^30], nseg
 * outside [0, TRUNET_WAVE_LOSS_MAX_SEG], n_items outside [1, 2 ceil(L/P) + nseg], a negative eps, a short or misaligned
 * workspace, or a written buffer overlapping any other. */
#define TRUNET_WAVE_LOSS_MAX_SEG 1024
#define TRUNET_WAVE_LOSS_PIECE 2048
typedef struct trunet_wave_loss_args {
    const float* audio;          /* x (B, L) */
    const float* clean;          /* y (B, L) */
    const int32_t* bounds;       /* (nseg + 1) */
    const int32_t* seg_first;    /* (nseg + 2) */
    const int32_t* items;        /* (n_items, 2) */
    int32_t B, L, nseg, n_items;
    double cos_lambda, si_sdr_lambda, cos_eps, si_sdr_eps;
} trunet_wave_loss_args;
size_t trunet_wave_loss_workspace_bytes(int B, int L, int nseg);
int trunet_wave_loss_fwd(const trunet_wave_loss_args* h_args, void* ws, size_t ws_bytes, float* vals, float* terms,
                         float* coef, float* loss_accum, void* stream);
int trunet_wave_loss_grad(const trunet_wave_loss_args* h_args, const float* coef, const float* g_loss, float* g_audio,
                          void* stream);

/* ======================================================================================================================
 * bf16 storage / bf16 MFMA family (BASELINE.json configs[2]; build extension: the reference has no reduced-precision path,
 * SURVEY 8d).  Activations and their gradients are stored as bf16 in the "octet" layout
 *     uint16 t[C/8][L][NP][8]      element (c, l, n) at (((c/8)*L + l)*NP + n)*8 + c%8
 * (channels padded to a multiple of 8 with zeros; NP a multiple of 64): a v_mfma_f32_32x32x16_bf16 B fragment -- 8
 * consecutive channels of one frame -- is ONE 16-byte load per lane, and taps / strides / pad / crop / cat stay whole-row
 * offsets as in the fp32 layout.  Accumulation, BatchNorm statistics (taken from the ROUNDED stored values, so forward and
 * backward see the same tensor), coefficients, weight gradients, master weights: fp32.
 * ====================================================================================================================== */
typedef struct {
    const void* src0;   /* bf16 octet tensor [ceil(nchan/8)][L][NP][8] */
    const void* src1;   /* second tensor for TRUNET_PRO_BNBWD */
    const float* c0; const float* c1; const float* c2;   /* per-channel coefficients [nchan] */
    int32_t nchan, L, pos_mul, pos_off, pos_div, mode;
    int32_t kstep0;     /* trunet_bf16_gemm: first 16-channel k-step of this segment in the packed weight image */
    int32_t woff;       /* trunet_bf16_wgrad: weight offset of this segment (as trunet_seg.woff) */
} trunet_bseg;
/* out[m][p + out_pos_off][n] = epi( sum_seg sum_c W(m, seg, c) * pro_seg(src_seg[c][q_seg(p)][n]) ), all tensors in the octet
 * layout, same prologue / epilogue flags as trunet_conv_gemm (network.py:13,28,50,64,67,83,86,106,109 and their data
 * gradients).  wfrag: the weight as packed by trunet_bf16_pack_weight ([row tile][k-step][64 lanes][8 bf16], MFMA A-fragment
 * order).  M <= 128.  Statistics partial rows: partials[trunet_bf16_gemm_nparts()][M_stat][2] (zero-filled by the call). */
typedef struct {
    int32_t NP, N, P, p_begin, M, out_L, out_pos_off, nseg, epi, M_stat, nks_total;
    int32_t m_out_off;        /* TRUNET_EPI_F32OUT: first output row of this launch in `out` (and in `bias`) */
    void* out; const void* wfrag; const float* bias; const void* zmask;
    const float* e0; const float* e1; const float* e2; float* partials;
    trunet_bseg seg[TRUNET_MAX_SEG];
} trunet_bgemm_args;
int trunet_bf16_gemm_nparts(void);
int trunet_bf16_gemm(const trunet_bgemm_args* h_args, void* stream);
/* the kernel instance trunet_bf16_gemm launches for these arguments (host only, no HIP call; the same argument checks and the
 * same return codes as the launch): bgemm_kernel<nrt, pro, epi, full>, pro / epi = -1 for the instances that test modes and
 * flags at run time.  full = 1 (no row or channel guards) needs M = 64 or 128 and every segment a multiple of 16 channels. */
int trunet_bf16_gemm_plan(const trunet_bgemm_args* h_args, int* nrt, int* pro, int* epi, int* full);
/* pack an fp32 weight into the A-fragment image: A(m, k) = W[(m + w_m_off)*ldw_m + c*ldw_c + h_seg_woff[s]] for segments of
 * h_seg_nchan[s] channels, each padded to whole k-steps of 16:
 * wfrag[((rt*nks_total + ks)*64 + lane)*8 + j] = A(32 rt + lane%32, 16 ks + 8 (lane/32) + j); returns nks_total (> 0) */
int trunet_bf16_pack_weight(const float* W, void* wfrag, int M, int ldw_m, int ldw_c, int w_m_off, int nseg,
                            const int32_t* h_seg_nchan, const int32_t* h_seg_woff, void* stream);
/* the same for a whole table of images in one launch: d_descs is a DEVICE array of n descriptors (ks0[s] = first k-step of segment s,
 * nks_total as trunet_bf16_pack_weight returns it), max_elems = max over the table of ceil(M/32) * nks_total * 64 */
typedef struct {
    const float* W; void* out;
    int32_t M, ldw_m, ldw_c, w_m_off, nseg, nks_total;
    int32_t nchan[TRUNET_MAX_SEG], woff[TRUNET_MAX_SEG], ks0[TRUNET_MAX_SEG];
    int32_t _pad;
} trunet_bpack_desc;
int trunet_bf16_pack_weights_batch(const trunet_bpack_desc* d_descs, int n, int max_elems, void* stream);
/* weight gradient of the same implicit GEMM from octet tensors: dW[(m+w_m_off)*ldw_m + c*ldw_c + woff_s] = sum_{p,n<N}
 * dz[m][p + a_pos_off][n] pro_s(src_s[c][q_s(p)][n]), dz = a0 (PRO_NONE) or ac0 a0 + ac1 a1 + ac2; fp32 partial images / bias
 * partial rows exactly as trunet_conv_wgrad (trunet_conv_wgrad_nparts() images, image stride w_numel).  M <= 128, at most 40
 * source octets over all segments.  A step is (position, 64 frames): every operand row is read from HBM once, transformed and
 * written to LDS as [octet][frame][8 channels]; the frame axis becomes the MFMA K axis through ds_read_b64_tr_b16. */
typedef struct {
    int32_t NP, N, P, p_begin, M, a_L, a_pos_off, a_mode, ldw_m, ldw_c, w_m_off, nseg, w_numel, b_stride, b_off, _pad;
    const void* a0; const void* a1; const float* ac0; const float* ac1; const float* ac2;
    float* w_partials; float* b_partials;
    trunet_bseg seg[TRUNET_MAX_SEG];
} trunet_bwgrad_args;
int trunet_bf16_wgrad(const trunet_bwgrad_args* h_args, void* stream);
/* Fused backward of a Conv1d(k=1)+BatchNorm layer on octet tensors (autograd of network.py:28,50,64,83 + :96-98): the weight /
 * bias gradient of trunet_bf16_wgrad AND, per source segment s, the data gradient
 *     dsrc_s[c][p + pos_off_s][n] = sum_m W[m][woff_s + c] dz[m][p][n]
 * in one pass over (dy, z, sources): flags[s] = TRUNET_DG_STORE | TRUNET_DG_MASK (zero where the source's BN+ReLU output is 0;
 * a plain post-ReLU source: where it is 0) | TRUNET_DG_STATS (sum dsrc, sum dsrc (z_s - mean[s]) over valid frames into
 * partials[s][trunet_bf16_pw_bwd_nparts()][nchan_s][2], zero-filled by the call) | TRUNET_DG_ACCUM (add to what out[s] holds).
 * wfragT: W^T as A fragments, sources' 32-channel row tiles one after the other, each packed by
 * trunet_bf16_pack_weight(W, ., nchan_s, 1, K, woff_s, 1, {M}, {0}); nrt_total = sum nchan_s / 32.
 * Restrictions (else TRUNET_ENOTSUP: use trunet_bf16_wgrad + trunet_bf16_gemm): a_mode = TRUNET_PRO_BNBWD, pos_mul = pos_div = 1,
 * nchan_s % 32 == 0, M % 16 == 0, at most 24 source octets, the LDS image within 160 KB. */
typedef struct {
    const void* wfragT;
    void* out[TRUNET_MAX_SEG];
    const float* mean[TRUNET_MAX_SEG];
    float* partials[TRUNET_MAX_SEG];
    int32_t flags[TRUNET_MAX_SEG];
    int32_t nrt_total;
} trunet_bdgrad_args;
typedef struct { trunet_bwgrad_args w; trunet_bdgrad_args dg; } trunet_bpwbwd_args;
int trunet_bf16_pw_bwd_nparts(void);
int trunet_bf16_pw_bwd(const trunet_bpwbwd_args* h_args, void* stream);
/* Fused backward of ConvTranspose1d(64 -> 64, K, S) + BatchNorm on octet tensors (autograd of network.py:67,86: decoder.0-4), the
 * bf16 counterpart of trunet_convt_bwd: one pass over (dy, z, source) with a sliding window of BatchNorm-backward-transformed
 * dz rows in LDS -> weight gradient W[ci][co][k] and bias gradient (fp32 partial images as trunet_conv_wgrad), the masked data
 * gradient dsrc[ci][q] of the pointwise BatchNorm's output and its BatchNorm-backward sums
 * partials[trunet_bf16_convt_bwd_nparts()][64][2] (zero-filled by the call).  wfragT = trunet_bf16_pack_weight(W, ., 64, Co*K, K,
 * 0, K, {64,..}, {0..K-1}).  Ci = Co = 64, (K, S) in {(3,1), (5,2), (3,2)}, pad = S/2 (else TRUNET_ENOTSUP). */
typedef struct {
    int32_t NP, N, Lin, Lout, K, S, pad, Ci, Co, w_numel, b_stride, b_off;
    int32_t prezero, _pad;    /* prezero != 0: `partials` is already zero (see TRUNET_EPI_PREZERO) */
    const void* dy; const void* z; const float* ca; const float* cb; const float* cc;
    const void* src; const float* s_scale; const float* s_shift; const float* s_mean;
    const void* wfragT; void* dsrc; float* partials; float* w_partials; float* b_partials;
} trunet_bconvt_args;
int trunet_bf16_convt_bwd_nparts(void);
int trunet_bf16_convt_bwd(const trunet_bconvt_args* h_args, void* stream);
/* depthwise conv in the octet layout (network.py:33-38; csrc/depthwise.hip): BN+ReLU prologue on the input, raw bf16 output, fp32 statistics
 * partials[trunet_bf16_dw_nparts(NP, rows)][C][2] (rows = Lout forward, Lin backward); backward: dz = ca dy + cb z + cc, masked
 * data gradient of the input (+ its BatchNorm-backward sums), fp32 partial images w_partials[nparts][C][K],
 * b_partials[nparts][C].  A thread owns (octet, frame) and walks positions with a sliding register window: every tensor is
 * read once.  (K, S) in {(3,1), (5,2), (3,2)}; C a multiple of 8. */
int trunet_bf16_dw_nparts(int NP, int rows);
int trunet_bf16_dwconv_fwd(const void* zin, const float* s_in, const float* t_in, const float* w, const float* b, void* zout,
                           float* partials, int C, int K, int S, int Lin, int Lout, int NP, int N, void* stream);
int trunet_bf16_dwconv_bwd(const void* dy, const void* z, const float* ca, const float* cb, const float* cc, const void* zin,
                           const float* s_in, const float* t_in, const float* mean_in, const float* w, void* dy_in,
                           float* partials_in, float* w_partials, float* b_partials, int C, int K, int S, int Lin, int Lout,
                           int NP, int N, void* stream);
/* The bidirectional GRU recurrence over L positions (trunet_gru_fwd / trunet_gru_bwd; network.py:48,55) on octet tensors:
 * gi [6H/8][L][NP][8] (both directions' input projections incl. b_ih, torch gate order r, z, n), hout / dhout / dghn
 * [2H/8][L][NP][8], gates [2][4][H/8][L][NP][8] (r, z, n, W_hn h + b_hn; NULL in eval), dgi like gi.  fp32 MFMAs and an
 * fp32 carry inside the recurrence; only the tensors in HBM are bf16.  H = 64 (TRUNET_ENOTSUP otherwise). */
int trunet_bf16_gru_fwd(const void* gi, const float* w_hh, const float* b_hh, const float* w_hh_rev, const float* b_hh_rev,
                        void* hout, void* gates, int H, int L, int NP, void* stream);
int trunet_bf16_gru_bwd(const void* dhout, const void* hout, const void* gates, const float* w_hh, const float* w_hh_rev,
                        void* dgi, void* dghn, int H, int L, int NP, void* stream);
/* layout changes: frames-last fp32 [C][L][NP] <-> octet bf16 (network input / output and the fp32 bottleneck of the bf16
 * path: FGRU); channels C..8*ceil(C/8)-1 of the octet tensor are written as zeros */
int trunet_bf16_from_frames_last(const float* x, void* y_oct, int C, int L, int NP, void* stream);
/* (N, C, L) fp32 of the module API <-> one octet [L][NP][8] directly (C <= 8: network input, output, output cotangent); frames
 * N..NP-1 and channels C..7 of the octet tensor are written as zeros */
int trunet_bf16_from_ncl(const float* x_ncl, void* y_oct, int N, int C, int L, int NP, void* stream);
int trunet_bf16_to_ncl(const void* y_oct, float* x_ncl, int N, int C, int L, int NP, void* stream);
int trunet_bf16_to_frames_last(const void* x_oct, float* y, int C, int L, int NP, void* stream);

/* calibration: sustained fp32 MFMA rate at the device's operating clock (out: blocks*256 floats) */
int trunet_debug_mfma_peak(float* out, int blocks, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
