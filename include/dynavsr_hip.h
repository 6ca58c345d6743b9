/*
 * dynavsr_hip.h -- C ABI of libdynavsr_hip.so: MI355X (gfx950) kernels for the EDVR hot path of
 * DynaVSR (PCD deformable alignment, TSA fusion, reconstruction) and its inner MAML step.
 *
 * Contract (all entry points):
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer on the current HIP device,
 *     fp32, contiguous NCHW unless stated; tensors are borrowed, never owned or freed;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream), no
 *     internal synchronisation, no allocation: scratch comes from a caller workspace;
 *   - returns 0 on success or a negative DVSR_ERR_* code and never throws; the message of the
 *     last failure on the calling thread is dvsr_last_error();
 *   - the stateless entry points are re-entrant (the only global mutable state is that thread-local error
 *     string).  PLAN objects (dvsr_edvr_plan, dvsr_estimator_plan) are NOT: a plan owns a side stream and
 *     fork/join events that its backward records on, so one plan must be driven by one host thread at a time
 *     (the reference's caller is single-threaded too: the autograd engine thread).  Different plans
 *     may be used from different threads concurrently.
 *
 * Each declaration cites the reference interface it replaces (paths under codes/ of
 * esw0116/DynaVSR).  The reference's only native boundary is the pybind11 module
 * `deform_conv_cuda` (models/archs/dcn/src/deform_conv_cuda.cpp:681-695); everything else the
 * reference gets from cuDNN/ATen through torch.nn, which these kernels replace one-for-one.
 */
#ifndef DYNAVSR_HIP_H_
#define DYNAVSR_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVSR_OK 0
#define DVSR_ERR_INVALID (-1)
#define DVSR_ERR_UNSUPPORTED (-2)
#define DVSR_ERR_WORKSPACE (-3)
#define DVSR_ERR_HIP (-4)

#define DVSR_ACT_NONE 0
#define DVSR_ACT_LRELU 1 /* LeakyReLU(0.1): models/archs/EDVR_arch.py:93,161,252 */
#define DVSR_ACT_RELU 2  /* models/archs/arch_util.py:50 */

typedef void* dvsr_stream_t; /* hipStream_t */

const char* dvsr_last_error(void);
int dvsr_version(void);

/* ---- modulated deformable convolution (DCNv2) ------------------------------------------------
 * Replaces modulated_deform_conv_cuda_forward (deform_conv_cuda.cpp:486-564; kernels
 * deform_conv_cuda_kernel.cu:466-496,569-632) with ONE fused kernel: bilinear sampling, mask
 * and the Cout x (C*kh*kw) contraction happen per tile in LDS/MFMA, no im2col buffer in HBM.
 *   x [N,C,H,W]  offset [N,dg*2*kh*kw,Ho,Wo] ((dy,dx) interleaved per tap)  mask [N,dg*kh*kw,Ho,Wo]
 *   w [Cout,C/groups,kh,kw]  b [Cout] or NULL  ->  out [N,Cout,Ho,Wo] (overwritten)
 * Supported: kh=kw=3, groups=1, C/dg in {4,8,16}; anything else returns DVSR_ERR_UNSUPPORTED
 * (the reference raises through AT_ERROR, cpp:506-511).  `act` is applied to the result
 * (EDVR_arch.py:103,126 apply LeakyReLU right after the DCN; pass DVSR_ACT_NONE for the op alone).
 */
int dvsr_mdcn_forward(const float* x, const float* offset, const float* mask, const float* w,
                      const float* b, float* out, int N, int C, int H, int W, int Cout, int kh,
                      int kw, int stride, int pad, int dil, int groups, int dg, int act,
                      dvsr_stream_t stream);

/* Fast path of dvsr_mdcn_forward for the EDVR configuration (3x3, stride = pad = dil = 1, groups = 1,
 * C/dg a multiple of 8 -- EDVR-M 64/8, EDVR-L 128/8): 8-channel slices of a deformable group's input planes
 * are staged in LDS and sampled from there (8 LDS
 * reads per (pixel, tap) instead of 32 global gathers); samples that leave the staged window
 * (|offset| > 4 px) fall back to exact global gathers.  The workspace receives the packed weights. */
size_t dvsr_mdcn_forward_fast_workspace_bytes(int C, int Cout, int dg);
int dvsr_mdcn_forward_fast(const float* x, const float* offset, const float* mask, const float* w,
                           const float* b, float* out, int N, int C, int H, int W, int Cout, int dg, int act,
                           void* workspace, size_t workspace_bytes, dvsr_stream_t stream);

/* Replaces modulated_deform_conv_cuda_backward (deform_conv_cuda.cpp:566-679).  grad_out = gradient
 * w.r.t. the op's output (act = NONE).  gx is ACCUMULATED into with fp32 atomics (zero it first, the
 * reference's caller does: deform_conv.py:128); goffset/gmask/gw/gb are overwritten; gx/gw/gb may
 * be NULL.  Workspace: the EDVR configuration (3x3, stride / pad / dilation 1, 8 channels per group) runs the fused
 * kernel, whose scratch is the per-workgroup [Cout][72] weight-gradient partials and (r06) the weights re-laid-out as the
 * kernel's first-phase operands, once per call (no column buffer: dcol and the sampled columns stay on chip; with Cout = 64,
 * W % 4 == 0 and 16-byte aligned x / grad_out both contractions run on the bf16 MFMA under the exact 3-way operand split:
 * fp32 results); other configurations take the three-kernel path, which also needs the [C*9, Ho*Wo] column buffer.
 * dvsr_mdcn_backward_workspace_bytes() returns the larger of the two. */
size_t dvsr_mdcn_backward_workspace_bytes(int N, int C, int H, int W, int Cout, int kh, int kw, int stride,
                                          int pad, int dil);
int dvsr_mdcn_backward(const float* x, const float* offset, const float* mask, const float* w,
                       const float* grad_out, float* gx, float* goffset, float* gmask, float* gw, float* gb,
                       int N, int C, int H, int W, int Cout, int kh, int kw, int stride, int pad, int dil,
                       int groups, int dg, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);

/* Same op fed by the RAW output `om` [N, 3*dg*kh*kw, Ho, Wo] of ModulatedDeformConvPack's
 * conv_offset_mask (deform_conv.py:274-291): offset = om[:, :2*dg*K], mask = sigmoid(om[:, 2*dg*K:]);
 * the chunk/cat/sigmoid launches of the reference are folded into the sampler. */
int dvsr_mdcn_pack_forward(const float* x, const float* om, const float* w, const float* b,
                           float* out, int N, int C, int H, int W, int Cout, int kh, int kw,
                           int stride, int pad, int dil, int groups, int dg, int act,
                           dvsr_stream_t stream);

/* dvsr_mdcn_forward_fast on `om` (offsets, then mask logits: the sigmoid is taken in the sampler): the kernels and the
 * kernel selection of the engine's DCN op -- on aligned tensors with W % 4 == 0 the bf16-pipe kernel under the exact 3-way
 * split, otherwise the register-staged fp32 one.  dvsr_mdcn_pack_forward above runs the generic gather kernel on every shape.
 * Workspace: dvsr_mdcn_forward_fast_workspace_bytes(). */
int dvsr_mdcn_pack_forward_fast(const float* x, const float* om, const float* w, const float* b, float* out, int N,
                                int C, int H, int W, int Cout, int dg, int act, void* workspace,
                                size_t workspace_bytes, dvsr_stream_t stream);

/* ---- dense convolution ------------------------------------------------------------------------
 * Replaces nn.Conv2d (+ the torch.cat feeding it, + the activation / residual add /
 * nn.PixelShuffle(2) following it) everywhere in EDVR_arch.py / arch_util.py:34-52.
 * LDS-staged implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), no im2col. */
typedef struct dvsr_conv2d_desc {
  const float* x0;   /* [N][c0][H][W] */
  const float* x1;   /* optional 2nd input, concatenated after x0 along C: [ceil(N/x1_bdiv)][c1][H][W]; NULL if c1==0 */
  const float* w;    /* [Cout][c0+c1][ks][ks] (OIHW) */
  const float* bias; /* [Cout] or NULL */
  const float* res;  /* optional tensor added AFTER the activation, shaped like y; NULL = none */
  float* y;          /* [N][Cout][Ho][Wo]; with pixel_shuffle=2: [N][Cout/4][2Ho][2Wo] */
  int N, c0, c1, H, W, Cout;
  int ks;            /* 1 or 3 */
  int stride;        /* 1 or 2 */
  int pad;           /* zero padding, must be ks/2 */
  int act;           /* DVSR_ACT_* applied to conv+bias */
  int pixel_shuffle; /* 0, or 2 = nn.PixelShuffle(2) fused into the store (EDVR_arch.py:247,303-305) */
  int x1_bdiv;       /* x1 batch index = n / x1_bdiv (>=1): one reference frame shared by N frames */
  long long x0_bstride; /* elements between batch items of x0; 0 = dense (c0*H*W) */
  long long x1_bstride; /* same for x1; 0 = dense (c1*H*W) */
  /* Optional addend BEFORE the activation: y = act(conv + bias + pre[n / pre_bdiv]), pre a dense fp32
   * [ceil(N/pre_bdiv)][Cout][Ho][Wo], 16-byte aligned; NULL = none (pre_bdiv <= 0 counts as 1).  By linearity it carries the
   * part of a two-input convolution whose input several batch items share -- conv_W(cat(f_i, ref)) = conv_W[:, :c0](f_i) +
   * conv_W[:, c0:](ref) -- computed once.  Only the packed Winograd F(4x4,3x3) kernel implements it: dvsr_conv2d_forward_packed
   * runs that kernel whenever the launch is eligible for it (aligned 3x3 / stride 1 / pad 1, W % 4 == 0, c0 and c1 multiples of
   * 8, at least 16 inputs and 32 outputs, no res, no pixel_shuffle) and returns DVSR_ERR_UNSUPPORTED otherwise, as
   * dvsr_conv2d_forward (no pack) and every other entry always do: the addend is never dropped. */
  const float* pre;
  int pre_bdiv;
} dvsr_conv2d_desc;

int dvsr_conv2d_forward(const dvsr_conv2d_desc* d, dvsr_stream_t stream);
/* Backward of the plain layout (pixel_shuffle=0, x1_bdiv<=1): `gy` = gradient w.r.t. the
 * PRE-activation output.  gx0/gx1/gw/gb may be NULL to skip; all are overwritten.  Data gradient =
 * the same MFMA kernel on the transposed, tap-mirrored weight view (zero-dilated for stride 2);
 * weight/bias gradient = split-K MFMA kernel + deterministic reduce (conv2d_wgrad.hip). */
size_t dvsr_conv2d_backward_workspace_bytes(const dvsr_conv2d_desc* d);
int dvsr_conv2d_backward(const dvsr_conv2d_desc* d, const float* gy, float* gx0, float* gx1, float* gw,
                         float* gb, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);

/* ---- streaming (HBM-bound) ops ------------------------------------------------------------------
 * F.interpolate(scale_factor=S, mode='bilinear', align_corners=False) * mul
 * (EDVR_arch.py:107-108,111,116-117,120,192,197,311); x [planes,H,W] -> y [planes,S*H,S*W]. */
int dvsr_upsample_bilinear_forward(const float* x, float* y, long long planes, int H, int W,
                                   int scale, float mul, dvsr_stream_t stream);
int dvsr_upsample_bilinear_backward(const float* gy, float* gx, long long planes, int H, int W,
                                    int scale, float mul, int accumulate, dvsr_stream_t stream);
/* nn.MaxPool2d(3,2,1) and nn.AvgPool2d(3,2,1) of the same tensor in one pass
 * (EDVR_arch.py:149-150,184-185,189-190). */
int dvsr_pool3s2_forward(const float* x, float* ymax, float* yavg, long long planes, int H, int W,
                         dvsr_stream_t stream);
int dvsr_pool3s2_backward(const float* x, const float* gmax, const float* gavg, float* gx,
                          long long planes, int H, int W, dvsr_stream_t stream);
/* TSA temporal attention gate (EDVR_arch.py:169-176): cor = sigmoid(sum_c emb*emb_ref) [B,N,HW],
 * gated = aligned * cor [B,N*C,HW]. */
int dvsr_tsa_gate_forward(const float* emb, const float* emb_ref, const float* aligned, float* cor,
                          float* gated, int B, int N, int C, long long HW, dvsr_stream_t stream);
int dvsr_tsa_gate_backward(const float* emb, const float* emb_ref, const float* aligned,
                           const float* cor, const float* g_gated, float* g_emb, float* g_emb_ref,
                           float* g_aligned, int B, int N, int C, long long HW,
                           dvsr_stream_t stream);
/* out = fea * sigmoid(att) * 2 + att_add (EDVR_arch.py:200-202). */
int dvsr_tsa_blend_forward(const float* fea, const float* att, const float* att_add, float* out,
                           long long n, dvsr_stream_t stream);
int dvsr_tsa_blend_backward(const float* fea, const float* att, const float* g, float* g_fea,
                            float* g_att_io, long long n, dvsr_stream_t stream);

/* ---- whole-network execution plan ----------------------------------------------------------------
 * Replaces `netG(var_L)` = EDVR.forward (models/archs/EDVR_arch.py:254-313, incl. PCD_Align :95-128
 * and TSA_Fusion :163-203) as called from VideoBaseModel.calculate_loss/test
 * (models/Video_base_model.py:191-201): one call enqueues every kernel of the backbone on `stream`.
 * `params` is a HOST array of dvsr_edvr_num_params() device pointers in the reference's state-dict
 * order (conv_first.weight, conv_first.bias, feature_extraction.0.conv1.weight, ... conv_last.bias).
 * x [B,nframes,3,H,W] -> out [B,3,scale*H,scale*W].  The workspace keeps every activation
 * (it is what a later backward call reads), so it must stay untouched between the two calls. */
typedef struct dvsr_edvr_config {
  int nf, nframes, groups, front_RBs, back_RBs, scale, center;
  /* 0: every contraction on the exact-fp32 MFMA (default; the parity configuration).
   * 1: the 3x3 stride-1 convolutions (forward and data gradient) round their operands to bf16 and run on
   *    v_mfma_f32_32x32x16_bf16 with fp32 accumulation; activations, weights, gradients, the DCN, the 1x1 /
   *    stride-2 convs and all weight gradients stay fp32 (BASELINE configs[4], "EDVR-L, bf16 MFMA path").
   * 2: experimental.  The same convolutions with every fp32 operand split exactly into three bf16 pieces
   *    (8 + 8 + 8 mantissa bits) and the six partial products above 2^-24 accumulated in fp32 on the bf16
   *    MFMA: fp32-level results (held to the fp32 parity bars by the tests), 6 x 32 instead of 8 x 64
   *    matrix-pipe cycles per 16 channels.  Not the default and not what bench.py's `value` is measured on. */
  int bf16_mfma;
} dvsr_edvr_config;
typedef struct dvsr_edvr_plan dvsr_edvr_plan;

int dvsr_edvr_plan_create(const dvsr_edvr_config* cfg, int B, int H, int W, dvsr_edvr_plan** out);
/* The same plan with PER-GROUP parameter gradients: the batch is `grad_groups` groups of B / grad_groups consecutive
 * clips, and dvsr_edvr_backward writes one gradient per group -- every grad_params[i] then points to
 * [grad_groups][numel(param i)] floats, group-major.  This is how the frames of a video that all adapt from the SAME
 * weights (test_dynavsr.py:208-277 deep-copies the un-adapted networks for every frame; with adapt_iter = 1, the value of
 * every shipped YAML, the K forward + backward passes differ only in their data) run as ONE batch of K clips whose
 * launches fill the device, while each frame still gets the gradient its own sequential step would have seen; the meta
 * tasks of train_dynavsr.py:355-426 likewise.  Forward, activations and data gradients are per sample in any case;
 * grad_groups = 1 is dvsr_edvr_plan_create.  The workspace grows by the extra weight-gradient partial sums. */
int dvsr_edvr_plan_create_grouped(const dvsr_edvr_config* cfg, int B, int H, int W, int grad_groups,
                                  dvsr_edvr_plan** out);
/* ... and PER-GROUP WEIGHTS (weight_sets == grad_groups; 1 = dvsr_edvr_plan_create_grouped): every params[i] then points to
 * [weight_sets][numel(param i)] floats and the clips of batch group g are convolved with set g, in forward, data gradient
 * and (per group, as above) weight gradient.  This is the K private copies of test_dynavsr.py:208 AFTER they have diverged:
 * the second and later inner steps (adapt_iter > 1: BASELINE configs[2] takes 3) and the adapted forwards of K frames
 * (:279-283) still run as one batch.  Every launch indexes its packed weights and bias by n / (N / weight_sets). */
int dvsr_edvr_plan_create_ex(const dvsr_edvr_config* cfg, int B, int H, int W, int grad_groups, int weight_sets,
                             dvsr_edvr_plan** out);
void dvsr_edvr_plan_destroy(dvsr_edvr_plan* plan);
int dvsr_edvr_num_params(const dvsr_edvr_plan* plan);
int dvsr_edvr_num_launches(const dvsr_edvr_plan* plan);
size_t dvsr_edvr_workspace_bytes(const dvsr_edvr_plan* plan, int need_grad);
int dvsr_edvr_forward(const dvsr_edvr_plan* plan, const float* const* params, const float* x,
                      float* out, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
/* dvsr_edvr_forward without its weight-packing launches, for a FROZEN network run over many clips (Video_base_model.py:197-201
 * `test()` called per clip of a video, test_dynavsr.py:200-204): `workspace` must be the workspace of an earlier
 * dvsr_edvr_forward of THIS plan with the SAME parameter values and the same need_grad sizing, not written by anyone since
 * (the packed weights live in it and are a pure function of the parameters).  Same launches otherwise, bit-identical
 * results.  After the parameters change, call dvsr_edvr_forward once again.  The caller owns that contract: stale packs are
 * not detected here (dynavsr_amd.engine keys them on the parameters' storage and version counters). */
int dvsr_edvr_forward_packed(const dvsr_edvr_plan* plan, const float* const* params, const float* x,
                             float* out, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
/* Backward of dvsr_edvr_forward (first-order; replaces autograd through EDVR incl. the 20 calls of
 * modulated_deform_conv_cuda_backward per clip, deform_conv_cuda.cpp:566-679).  Must follow a forward
 * on the SAME workspace, which must have been sized with need_grad=1.  grad_out [B,3,sH,sW];
 * grad_params: HOST array of device pointers shaped like `params`, every entry is OVERWRITTEN;
 * grad_x [B,nframes,3,H,W] or NULL.  The DCN input gradient uses fp32 atomics (summation order
 * varies run to run, as in the reference kernel, deform_conv_cuda_kernel.cu:687). */
int dvsr_edvr_backward(const dvsr_edvr_plan* plan, const float* const* params, const float* x,
                       const float* grad_out, float* const* grad_params, float* grad_x, void* workspace,
                       size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_edvr_num_backward_launches(const dvsr_edvr_plan* plan);
/* Measurement aids: per-launch description (kind = "conv3x3s1", "mdcn", ...; algorithmic FLOPs and
 * bytes of that launch) and a forward that brackets every launch with hipEvents on `stream`,
 * synchronises, and returns per-launch milliseconds in op_ms[dvsr_edvr_num_launches()]. */
int dvsr_edvr_op_info(const dvsr_edvr_plan* plan, int index, char* kind, int kind_cap, char* name,
                      int name_cap, double* flops, double* bytes);
/* Contraction work of the plan's two tapes: out9 (NINE doubles) = {forward algorithmic FLOPs, forward fp32 products as the
 * kernels shape them, backward algorithmic, backward shaped, algorithmic bytes of the forward tape (every launch's distinct
 * inputs once + its outputs once), forward FLOPs issued to the fp32 matrix pipe, forward FLOPs issued to the bf16 matrix pipe,
 * backward fp32-pipe, backward bf16-pipe}.  Algorithmic = 2 x MACs of the direct sums; launches on the Winograd
 * F(2x2,3x3) kernels do 16/36 of theirs; launches on the exact 3-way bf16 operand split issue six bf16 products per fp32
 * product.  bench.py's roofline fractions price the issued figures against the peak of the pipe they were issued to. */
int dvsr_edvr_plan_work(const dvsr_edvr_plan* plan, double* out9);
/* The same nine figures with the FORWARD tape priced as dvsr_edvr_forward runs it on a workspace WITHOUT the gradient region
 * (workspace_bytes < dvsr_edvr_workspace_bytes(plan, 1): test(), Video_base_model.py:197-201): such a forward may run the
 * Winograd F(4x4,3x3) kernel (36/144 of the direct sum's multiplies, six bf16 products each) on layers whose training tape
 * keeps F(2x2,3x3); dvsr_edvr_op_info's tags ("w5") and dvsr_edvr_forward_timed describe that forward. */
int dvsr_edvr_plan_work_nograd(const dvsr_edvr_plan* plan, double* out9);
/* Kernels that forward launch `index` issues for its own work: 2 for a two-input 3x3 convolution that a no-grad forward
 * (nograd != 0) runs as reference part + main part -- the half whose input the frames of a clip share is convolved once per
 * clip and enters the other half's epilogue as an addend; DVSR_PCD_HOIST=0 at plan creation keeps it one launch -- and 1 for
 * everything else (also for the two 1x1 convolutions that may share one launch: that is settled when they run).  The op list,
 * its names and tags and the algorithmic figures of dvsr_edvr_op_info do not change with it; dvsr_edvr_forward_timed times
 * both kernels under the launch.  -1: bad argument. */
int dvsr_edvr_op_launch_count(const dvsr_edvr_plan* plan, int index, int nograd);
/* Does the plans' weight-gradient side stream run BESIDE `stream` on the current device?  ROCm maps HIP streams onto
 * GPU_MAX_HW_QUEUES hardware queues and two streams on one queue serialise -- which queue a stream gets depends on every
 * stream the process created before (an initialised RCCL communicator holds some; train_dynavsr.py:23-30 creates it first).
 * Measured once per (device, stream) with a 150 us two-kernel probe and cached: 1 overlaps, 0 serialised (dvsr_edvr_backward /
 * dvsr_estimator_backward then launch their weight gradients on `stream` itself instead of forking), -1 unknown (the stream is
 * being captured, or DVSR_BWD_PROBE=0).  Synchronises `stream`. */
int dvsr_side_stream_overlaps(dvsr_stream_t stream);
/* Test aid: where launch `index` of the forward tape leaves its result (which = 0; 1 = the second output of the pool /
 * TSA-gate launches).  *in_arena = 1: offset_floats counts from the start of the workspace (every activation of a
 * need_grad forward stays there); 0: the launch writes the output tensor. */
int dvsr_edvr_op_output(const dvsr_edvr_plan* plan, int index, int which, int* in_arena, long long* offset_floats,
                        long long* numel);
int dvsr_edvr_forward_timed(const dvsr_edvr_plan* plan, const float* const* params, const float* x,
                            float* out, void* workspace, size_t workspace_bytes,
                            dvsr_stream_t stream, float* op_ms);
/* Measurement aid: register-only fp32 MFMA loop (256-thread workgroups, `nacc` accumulators per wave,
 * `lds_bytes` of dynamic LDS to reproduce an occupancy); returns MFMA instructions per wave or -1. */
long long dvsr_debug_mfma_peak(float* out, int blocks, int iters, int nacc, int lds_bytes, dvsr_stream_t stream);
/* Measurement aid (tools/mfma_shadow.py): shader cycles of a stream of fp32 MFMAs with nv v_fma_f32 (kind 0) or
 * ds_read_b32 (kind 1) behind each one, accumulators in VGPRs (acc 0) or AGPRs (acc 1). */
int dvsr_debug_mfma_shadow(long long* cycles, float* out, int blocks, int iters, int nv, int kind, int acc,
                           dvsr_stream_t stream);
/* Offset (in floats, into the workspace) and size of a named intermediate, for layer-by-layer
 * parity checks ("L1_fea", "aligned", "tsa_out", "recon", ...). */
int dvsr_edvr_tensor_info(const dvsr_edvr_plan* plan, const char* name, long long* offset_floats,
                          long long* numel);

/* ---- Streaming EDVR forward: every frame's features extracted ONCE ----------------------------
 * A video is super-resolved over a sliding window of `nframes` frames (test_dynavsr.py:200-204 per window of
 * data/util.py:index_generation), and the launches of EDVR.forward up to L3_fea (EDVR_arch.py:272-279: conv_first, the
 * front residual blocks, fea_L2_conv*, fea_L3_conv*) depend on one frame each: consecutive windows recompute them for the
 * frames they share.  A stream object splits the B = 1 no-grad tape at L3_fea:
 *   extract: one LR frame [3][H][W] -> its L1 / L2 / L3 features + the frame itself, written into slot `slot` of a
 *            caller-owned cache of `slots` slots (dvsr_edvr_stream_cache_bytes);
 *   fuse:    `slots[nframes]` (HOST array, window order) -> out [3][scale*H][scale*W]: one gather launch copies the
 *            window's features out of the cache, then the tape runs from L3_offset_conv1 to conv_last unchanged.
 * Both tapes come from the walk that builds dvsr_edvr_plan (same parameter order: `params` is the same host array of
 * dvsr_edvr_stream_num_params() device pointers) and ALWAYS run the no-grad launch geometries -- the mode is this entry
 * point, not a workspace size.  cfg.bf16_mfma is respected.  At most DVSR_STREAM_MAX_FRAMES frames per window.
 * Workspace: dvsr_edvr_stream_workspace_bytes() per window in flight, shared by the extract and fuse calls made on that
 * window's HIP stream (it holds both tapes' activations and packed weights, in disjoint regions).
 * packed != 0: the contract of dvsr_edvr_forward_packed, per tape -- this workspace still holds the packs an earlier
 * extract (resp. fuse) call with packed = 0 left there for the same parameter values.
 * Ordering is the caller's: a fuse must be ordered behind the extractions of its slots, an extract behind every fuse
 * that still reads the slot it overwrites (the cache is read by the gather launch only, i.e. at the START of a fuse).
 * Bad arguments (null pointer, slot outside [0, slots), short or misaligned workspace / cache) return DVSR_ERR_INVALID
 * before any launch. */
#define DVSR_STREAM_MAX_FRAMES 16
typedef struct dvsr_edvr_stream dvsr_edvr_stream;
int dvsr_edvr_stream_create(const dvsr_edvr_config* cfg, int H, int W, int slots, dvsr_edvr_stream** out);
void dvsr_edvr_stream_destroy(dvsr_edvr_stream* stream_plan);
int dvsr_edvr_stream_num_params(const dvsr_edvr_stream* stream_plan);
/* launches of the extract (which = 0; + one device copy of the frame) / fuse (which = 1; gather included) tape */
int dvsr_edvr_stream_num_launches(const dvsr_edvr_stream* stream_plan, int which);
size_t dvsr_edvr_stream_cache_bytes(const dvsr_edvr_stream* stream_plan);
size_t dvsr_edvr_stream_workspace_bytes(const dvsr_edvr_stream* stream_plan);
/* The largest tensor that one image of a batch occupies, in bytes, over the ops of both tapes (numel / N * 4; an op without a
 * batch dimension counts as one image).  The conv and DCN kernels address one image of an NCHW tensor through a raw buffer
 * resource with 32-bit offsets: a plan for which this reaches 2^32 must not be run.  Host code, no device call. */
unsigned long long dvsr_edvr_stream_max_image_bytes(const dvsr_edvr_stream* stream_plan);
int dvsr_edvr_stream_extract(const dvsr_edvr_stream* stream_plan, const float* const* params, const float* frame, int slot,
                             void* cache, size_t cache_bytes, void* workspace, size_t workspace_bytes, int packed,
                             dvsr_stream_t stream);
int dvsr_edvr_stream_fuse(const dvsr_edvr_stream* stream_plan, const float* const* params, const int* slots,
                          const void* cache, size_t cache_bytes, float* out, void* workspace, size_t workspace_bytes,
                          int packed, dvsr_stream_t stream);

/* ---- Frames in and out of the video path ---------------------------------------------------------
 * What a decoder delivers and an encoder takes (8-bit interleaved RGB / BGR at any size, address and row pitch), to and
 * from what the network computes on (fp32 planar [3][H][W] in [0,1], H and W multiples of 4).  Replaces, per frame,
 * `img.astype(np.float32) / 255.` + BGR -> RGB + HWC -> CHW (data/util.py:82, :109) on the way in and the fp32
 * device -> host copy + util.tensor2img (utils/util.py:112-142) on the way out.
 * dvsr_frame_desc describes the frame on the "any address, any pitch" side:
 *   DVSR_FRAME_F32_CHW      fp32 planar; row_stride and plane_stride in FLOATS, columns contiguous, 4-byte aligned;
 *                           pixel_stride is ignored
 *   DVSR_FRAME_U8_HWC_RGB / _BGR   8-bit interleaved; row_stride in BYTES, pixel_stride 3 or 4 bytes (a fourth byte is
 *                           ignored; an emitted frame has pixel_stride 3); plane_stride is ignored
 * dvsr_frame_ingest: src (h x w) -> dst fp32 planar [3][Hp][Wp] RGB, Hp >= h, Wp >= w, Wp % 4 == 0, dst 16-byte aligned.
 *   8-bit values become v / 255.0f (correctly rounded, numpy's result).  Rows h .. Hp-1 and columns w .. Wp-1 are filled from
 *   the frame: DVSR_FRAME_PAD_REFLECT = torch.nn.functional.pad(x, (0, Wp-w, 0, Hp-h), 'reflect') (no edge repeat; needs
 *   Hp - h < h and Wp - w < w), DVSR_FRAME_PAD_REPLICATE = mode 'replicate'.
 * dvsr_frame_emit: src fp32 planar [3][Hs][Ws] (16-byte aligned, Ws % 4 == 0) -> its top-left dd->h x dd->w crop in
 *   dd->format at dst.  8-bit: clamp to [lo,hi], rescale, x 255, round half to even -- the quantiser of
 *   dvsr_frame_metrics, i.e. util.tensor2img(.., min_max=(lo,hi)) bit for bit on finite inputs (BGR = its mode 'bgr').
 *   F32_CHW: the plain crop (lo, hi unused).  Bytes between rows and behind the last row are not written.
 * dvsr_edvr_stream_extract_frame: dvsr_frame_ingest straight into the raw-frame section of cache slot `slot` (the stream
 *   plan's H x W are the padded size, the descriptor carries the true one), then the extract tape reading it there: the
 *   bits of dvsr_frame_ingest into a temporary + dvsr_edvr_stream_extract, without the temporary and the device copy.
 * Bad arguments (null pointer, unknown format / pad mode, h or w < 1 or beyond the target, a reflect pad not smaller than
 * the dimension, pixel stride outside {3,4}, a row stride shorter than a row, a misaligned fp32 side) return
 * DVSR_ERR_INVALID before any launch. */
#define DVSR_FRAME_F32_CHW 0
#define DVSR_FRAME_U8_HWC_RGB 1
#define DVSR_FRAME_U8_HWC_BGR 2
#define DVSR_FRAME_PAD_REFLECT 0
#define DVSR_FRAME_PAD_REPLICATE 1
typedef struct dvsr_frame_desc {
  int format;   /* DVSR_FRAME_* */
  int h, w;     /* the frame's own size */
  long long row_stride, plane_stride;
  int pixel_stride;
} dvsr_frame_desc;
int dvsr_frame_ingest(const void* src, const dvsr_frame_desc* sd, float* dst, int Hp, int Wp, int pad_mode,
                      dvsr_stream_t stream);
int dvsr_frame_emit(const float* src, int Hs, int Ws, void* dst, const dvsr_frame_desc* dd, float lo, float hi,
                    dvsr_stream_t stream);
int dvsr_edvr_stream_extract_frame(const dvsr_edvr_stream* stream_plan, const float* const* params, const void* frame,
                                   const dvsr_frame_desc* fd, int pad_mode, int slot, void* cache, size_t cache_bytes,
                                   void* workspace, size_t workspace_bytes, int packed, dvsr_stream_t stream);

/* ---- Scene cuts: the luma difference of consecutive frames ----------------------------------------
 * dvsr_frame_luma_sad: sad[i] = sum over the h x w frame of |Y8_b(p) - Y8_a(p)| for pair i = 0 .. pairs - 1, frame a of
 *   the pair at a + i * frame_stride and frame b at b + i * frame_stride (frame_stride in the descriptor's own units: bytes
 *   for the 8-bit formats, floats for F32_CHW; any value).  A device-resident video [T][...] is ONE call: b = a +
 *   frame_stride, pairs = T - 1.  Both frames of every pair share the descriptor.  Y8, the luma of a pixel, is an 8-bit integer:
 *     DVSR_FRAME_U8_Y                a single 8-bit plane (the Y plane of an NV12 / I420 frame, any address and row pitch,
 *                                    pixel_stride 1): the byte itself
 *     DVSR_FRAME_U8_HWC_RGB / _BGR   (pixel_stride 3 or 4)  Y8 = (77 R + 150 G + 29 B + 128) >> 8
 *     DVSR_FRAME_F32_CHW             the same formula on the 8-bit values of dvsr_frame_emit with lo = 0, hi = 1 (clamp, x 255,
 *                                    round half to even) of the three channels
 *   The sums are exact unsigned 64-bit integers and do not depend on the launch geometry.  The function zeroes sad[0 .. pairs)
 *   on `stream` itself, then launches (one launch per 65535 pairs); sad must be 8-byte aligned device memory.
 *     DVSR_FRAME_U16_Y_MSB / _10 / _12  a single plane of 16-bit little-endian words (the Y plane of a P010 / P012, a
 *                                    yuv420p10le, a yuv420p12le frame; 2-byte aligned, pixel_stride 2, row_stride and
 *                                    frame_stride in BYTES and even): the top 8 bits of the level, word >> 8,
 *                                    (word & 1023) >> 2, (word & 4095) >> 4 -- scores mean what they mean for 8-bit video
 *   DVSR_FRAME_U8_Y and DVSR_FRAME_U16_Y_* are accepted here and by dvsr_frame_score alone: dvsr_frame_ingest / _emit keep
 *   rejecting them.
 * Bad arguments (null pointer, unknown format, h or w < 1, pairs < 1, a pixel stride the format does not have, a row or
 * plane stride shorter than a row / plane, a misaligned fp32 frame or result, an odd address or stride of a 16-bit plane)
 * return DVSR_ERR_INVALID before any launch. */
#define DVSR_FRAME_U8_Y 3
#define DVSR_FRAME_U16_Y_MSB 4
#define DVSR_FRAME_U16_Y_10 5
#define DVSR_FRAME_U16_Y_12 6
int dvsr_frame_luma_sad(const void* a, const void* b, const dvsr_frame_desc* desc, long long frame_stride, int pairs,
                        unsigned long long* sad, dvsr_stream_t stream);

/* ---- 16-bit RGB and planar integer RGB / GBR frames -------------------------------------------------
 * What 16-bit PNG / TIFF / DPX readers and writers, torchvision's decoders (uint8 / uint16 [3,H,W]), an FFV1 archive (gbrp,
 * gbrp10le, gbrp12le, gbrp16le) and lossless 4:4:4 RGB codecs deliver and take: further values of dvsr_frame_desc.format for
 * dvsr_frame_ingest, dvsr_frame_emit, dvsr_edvr_stream_extract_frame, dvsr_frame_luma_sad and dvsr_frame_score -- no new entry
 * point, no new struct.  dvsr_frame_degrade, dvsr_frame_imresize, dvsr_task_degrade and dvsr_task_gather keep refusing them.
 *   DVSR_FRAME_U16_HWC_RGB / _BGR   16-bit little-endian words interleaved (rgb48le / bgr48le; pixel_stride 8: rgba64le /
 *                                   bgra64le, the fourth word ignored; an emitted frame has pixel_stride 6).  Depth 16.
 *   DVSR_FRAME_U8_CHW_RGB / _GBR    three byte planes [3][h][w] in the order R, G, B (a decoded image) or G, B, R (gbrp)
 *   DVSR_FRAME_U16_CHW_RGB / _GBR   three planes of 16-bit little-endian words; the level of d bits is in the LOW bits of a word,
 *                                   higher bits are ignored on the way in and written as 0.  d is part of the format:
 *                                   DVSR_FRAME_DEPTH(format, d), d = 10, 12 or 16 (16 is stored as 0: the bare value).
 * Units follow the 16-bit Y planes above: row_stride and plane_stride (planar formats; ignored for interleaved ones) in BYTES,
 * pixel_stride in bytes -- 6 or 8 for interleaved words, 1 / 2 for byte / word planes; addresses and strides of words are even.
 * Planes may lie at any plane_stride >= (h - 1) row_stride + a row.
 * Arithmetic, top = 2^d - 1 (exact in fp32):
 *   ingest   level = word & top (the word itself at depth 16, the byte at depth 8); value = (float)level / (float)top, an IEEE
 *            division (numpy's np.float32(level) / np.float32(top); depth 8: v / 255.0f, the bits of the 8-bit formats); GBR
 *            planes and BGR words go to R, G, B; padding as for every format, on the source index
 *   emit     t = (fminf(fmaxf(v, lo), hi) - lo) / (hi - lo), level = (int)rintf(t * (float)top): the 8-bit quantiser with 255
 *            replaced by top, round half to even.  Nothing outside the rows of the crop is written.
 *   luma_sad the 8-bit rule on the top 8 bits of each level: (77 R' + 150 G' + 29 B' + 128) >> 8 with X' = level >> (d - 8)
 *   score    channel rgb alone at d > 8 (the reference defines no Y from RGB there), on the d-bit levels with L = top;
 *            dvsr_score_args.depth = d, which then also quantises an fp32 side; both sides hold one depth
 * Bad arguments -- an unknown depth, an odd address or stride of a word frame, a row or plane stride shorter than a row or plane,
 * a pixel stride the format does not have (emit: 8) -- return DVSR_ERR_INVALID before any launch.
 * Not provided: separately allocated planes, rgb24-in-int32 / x2rgb10 / r210 packed words, big-endian words, float16 / float32
 * interleaved, an alpha plane or alpha out. */
#define DVSR_FRAME_U16_HWC_RGB 16
#define DVSR_FRAME_U16_HWC_BGR 17
#define DVSR_FRAME_U8_CHW_RGB 18
#define DVSR_FRAME_U8_CHW_GBR 19
#define DVSR_FRAME_U16_CHW_RGB 20
#define DVSR_FRAME_U16_CHW_GBR 21
#define DVSR_FRAME_DEPTH(format, d) ((format) | (((d) & 15) << 8))   /* e.g. gbrp10le = DVSR_FRAME_DEPTH(DVSR_FRAME_U16_CHW_GBR, 10) */

/* ---- YCbCr 4:2:0 frames in and out of the video path -----------------------------------------------
 * What a video decoder really delivers and an encoder takes: 8-bit YCbCr 4:2:0 as NV12 or planar I420 (yuv420p), every plane
 * at any address and row pitch (row_stride in BYTES), chroma planes Hc x Wc = ceil(h/2) x ceil(w/2).  Converted on the
 * device, to and from the fp32 planar RGB [3][H][W] in [0,1] of the section above, without an 8-bit RGB frame in between.
 *   matrix  DVSR_YUV_BT601: Kr = 0.299, Kb = 0.114; DVSR_YUV_BT709: Kr = 0.2126, Kb = 0.0722; Kg = 1 - Kr - Kb
 *   range   DVSR_YUV_LIMITED: y0 = 16, ys = 219, cs = 224; DVSR_YUV_FULL: y0 = 0, ys = 255, cs = 255
 *   (BT601 + LIMITED: the reference's ycbcr2rgb / rgb2ycbcr, data/util.py:234-299.)  Chroma siting is the MPEG-2 / H.264
 *   default: chroma sample (j, k) on luma column 2k, midway between luma rows 2j and 2j+1.
 * dvsr_frame_ingest_yuv: sd (h x w) -> dst fp32 planar [3][Hp][Wp] RGB (as dvsr_frame_ingest: Wp % 4 == 0, 16-byte aligned,
 *   the same two pad modes, defined on the source index).  Chroma is brought to the luma grid by [1,1]/2 between two chroma
 *   columns (odd x) and 0.75 / 0.25 between the two nearest chroma rows, edges clamped; then yn = (Y - y0) / ys,
 *   c = (C - 128) / cs, R = yn + 2(1-Kr) cr, G = yn - (2 Kb (1-Kb) / Kg) cb - (2 Kr (1-Kr) / Kg) cr, B = yn + 2(1-Kb) cb,
 *   clamped to [0,1] and NOT rounded to 8 bits.
 * dvsr_frame_emit_yuv: src fp32 planar [3][Hs][Ws] -> its top-left dd->h x dd->w crop as 4:2:0 bytes: t = (clamp(v, lo, hi)
 *   - lo) / (hi - lo), y = Kr R + Kg G + Kb B, cb = (B - y) / (2(1-Kb)), cr = (R - y) / (2(1-Kr)); luma byte = clamp(rint(y0 +
 *   ys y), 0, 255); chroma sample (j, k) = taps [1,2,1]/4 on columns 2k-1 .. 2k+1, mean of rows 2j and 2j+1, indices clamped
 *   to the crop; chroma byte = clamp(rint(128 + cs c), 0, 255).  Bytes outside the rows of the planes are not written.
 * dvsr_edvr_stream_extract_frame_yuv: dvsr_edvr_stream_extract_frame for such a frame (no temporary, no device copy).
 * Bad arguments (null descriptor / plane, unknown format / matrix / range / pad mode, h or w < 1 or beyond the target, a row
 * stride shorter than a row, a reflect pad not smaller than the dimension, a misaligned fp32 side) return DVSR_ERR_INVALID
 * before any launch.
 *
 * 4:2:2 and 4:4:4 (ProRes / DNxHR / XAVC intermediates and capture surfaces; screen recordings, Hi444 / RExt, animation
 * masters): new values of `format` for the same functions and for those of the 16-bit section below -- the form (semi-planar
 * 0 | planar 1) in the low four bits, the sub-sampling above them: format = DVSR_YUV_FORMAT(form, chroma).  Chroma planes:
 *   DVSR_YUV_CHROMA_420  Hc x Wc = ceil(h/2) x ceil(w/2)   (0: the two forms alone are NV12 / I420, as they always were)
 *   DVSR_YUV_CHROMA_422  Hc x Wc = h x ceil(w/2)           nv16 / yuv422p; p210le / p212le / yuv422p10le / yuv422p12le
 *   DVSR_YUV_CHROMA_444  Hc x Wc = h x w, planar alone     yuv444p; yuv444p10le / yuv444p12le
 * Matrices, ranges, level scales, word conventions, clamps and roundings are those of 4:2:0; only the resampling differs.
 * 4:2:2: chroma sample (y, k) sits on luma row y, column 2k; ingest takes the [1,1]/2 step between two chroma columns and no
 * vertical step; emit takes the taps [1,2,1]/4 on columns 2k-1 .. 2k+1 of row y, clamped to the crop, and no vertical mean.
 * 4:4:4: a pixel's chroma is its own sample both ways.  A row stride must hold Wc samples (planar) or 2 Wc (semi-planar).
 * Not provided: semi-planar 4:4:4 (nv24 / p410: refused as an unknown format), packed 4:2:2 (YUY2 / UYVY / v210), 4:1:1 /
 * 4:4:0, depth 16 (YCbCr).  (Planar GBR: the RGB section above.)
 *
 * Chroma siting and BT.2020.  The chroma field of `format` names a pair of sub-sampling and siting:
 *   DVSR_YUV_CHROMA_420 (0), _422 (1)   "left": MPEG-2 / H.264 / y4m 420mpeg2, as always
 *   DVSR_YUV_CHROMA_420_CENTER (4), DVSR_YUV_CHROMA_422_CENTER (6)   JPEG / MPEG-1 / MJPEG, ffmpeg's yuvj420p, y4m 420jpeg
 *   DVSR_YUV_CHROMA_420_TOPLEFT (5)     HEVC / AV1 UHD and HDR10, chroma_sample_location=topleft (BT.2100)
 * Value 3, values above 6 and any bit above bit 7 are refused as an unknown format; plane sizes, forms and everything else are
 * those of the sub-sampling.  Chroma sample (j, k) sits at luma position (4:2:2: y is the luma row itself)
 *             x          y
 *   left      2k         2j + 1/2
 *   center    2k + 1/2   2j + 1/2
 *   topleft   2k         2j
 * ingest: linear interpolation at the luma pixel's position, indices clamped to the plane, k = x >> 1, j = y >> 1.  Horizontal
 *   step H(j, x): co-sited (left, topleft) as above; center: 0.75 C[j][k] + 0.25 C[j][max(k-1, 0)] (x even) |
 *   0.75 C[j][k] + 0.25 C[j][min(k+1, Wc-1)] (x odd).  Vertical step (4:2:0): midway (left, center) as above; co-sited
 *   (topleft): H(j, x) (y even) | (H(j, x) + H(min(j+1, Hc-1), x)) / 2 (y odd).
 * emit: filters centred on the chroma sample's position, indices clamped to the crop.  Horizontal: co-sited [1,2,1]/4 on
 *   2k-1, 2k, 2k+1 as above; center: the mean of columns 2k and min(2k+1, w-1).  Vertical (4:2:0): midway the mean of rows 2j
 *   and min(2j+1, h-1) as above; co-sited: [1,2,1]/4 on rows max(2j-1, 0), 2j, min(2j+1, h-1).  Luma does not depend on siting.
 * DVSR_YUV_BT2020NC (9, H.273's MatrixCoefficients code; 2 .. 8 stay refused): BT.2020 non-constant luminance, Kr = 0.2627,
 * Kb = 0.0593, with the ranges and level scales of the other two.  Not provided: constant-luminance BT.2020, ICtCp, transfer
 * functions (PQ / HLG: the network sees the transfer-coded R'G'B' as it does for SDR), a siting per direction, bottom and
 * interlaced sitings, 420paldv. */
#define DVSR_YUV_NV12 0      /* plane[0] = Y [h][w], plane[1] = CbCr interleaved [Hc][Wc][2]; plane[2] ignored */
#define DVSR_YUV_I420 1      /* plane[0] = Y, plane[1] = Cb [Hc][Wc], plane[2] = Cr [Hc][Wc] */
#define DVSR_YUV_CHROMA_420 0
#define DVSR_YUV_CHROMA_422 1
#define DVSR_YUV_CHROMA_444 2
#define DVSR_YUV_CHROMA_420_CENTER 4
#define DVSR_YUV_CHROMA_420_TOPLEFT 5
#define DVSR_YUV_CHROMA_422_CENTER 6
#define DVSR_YUV_FORMAT(form, chroma) ((form) | ((chroma) << 4))   /* e.g. nv16 = DVSR_YUV_FORMAT(DVSR_YUV_NV12, DVSR_YUV_CHROMA_422) */
#define DVSR_YUV_BT601 0
#define DVSR_YUV_BT709 1
#define DVSR_YUV_BT2020NC 9  /* Kr = 0.2627, Kb = 0.0593 */
#define DVSR_YUV_LIMITED 0
#define DVSR_YUV_FULL 1
typedef struct dvsr_yuv_desc {
  int format;   /* DVSR_YUV_NV12 / _I420, or DVSR_YUV_FORMAT(one of them, DVSR_YUV_CHROMA_*) */
  int h, w;     /* the frame's own (luma) size */
  int matrix, range;
  void* plane[3];
  long long row_stride[3];   /* bytes */
} dvsr_yuv_desc;
int dvsr_frame_ingest_yuv(const dvsr_yuv_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream);
int dvsr_frame_emit_yuv(const float* src, int Hs, int Ws, const dvsr_yuv_desc* dd, float lo, float hi, dvsr_stream_t stream);
int dvsr_edvr_stream_extract_frame_yuv(const dvsr_edvr_stream* stream_plan, const float* const* params, const dvsr_yuv_desc* fd,
                                       int pad_mode, int slot, void* cache, size_t cache_bytes, void* workspace,
                                       size_t workspace_bytes, int packed, dvsr_stream_t stream);

/* ---- 10- and 12-bit YCbCr 4:2:0 frames in and out of the video path --------------------------------
 * What an HEVC Main10 / AV1 / VP9 profile 2 decoder delivers and a 10-bit encoder takes: 16-bit little-endian words holding
 * depth = 10 or 12 bits, every plane at any 2-byte aligned address and any even row pitch (row_stride in BYTES), chroma planes
 * Hc x Wc = ceil(h/2) x ceil(w/2):
 *   DVSR_YUV16_SEMI_MSB    P010 / P012: word = level << (16 - depth); the low bits are ignored on the way in and written as 0
 *   DVSR_YUV16_PLANAR_LSB  yuv420p10le / yuv420p12le: word = level; the high bits are ignored on the way in and written as 0
 * The arithmetic is that of the 8-bit section above (matrix, siting, the two resampling filters, padding on the source index,
 * RGB clamped to [0,1], round half to even) with the level scale of H.273 at that depth, s = 2^(depth-8):
 *   DVSR_YUV_LIMITED: y0 = 16 s, ys = 219 s, cs = 224 s, chroma mid 128 s;  DVSR_YUV_FULL: y0 = 0, ys = cs = 2^depth - 1,
 *   chroma mid 2^(depth-1);  an emitted level is clamped to [0, 2^depth - 1].
 * dvsr_frame_ingest_yuv16 / dvsr_frame_emit_yuv16 / dvsr_edvr_stream_extract_frame_yuv16 are dvsr_frame_ingest_yuv /
 * dvsr_frame_emit_yuv / dvsr_edvr_stream_extract_frame_yuv for such a frame: one launch each, nothing rounded to 8 bits in
 * between, no temporary and no device copy on the way into the frame cache.
 * Bad arguments (null descriptor / plane, unknown format / depth / matrix / range / pad mode, h or w < 1 or beyond the target, a
 * row stride shorter than a row or odd, an odd plane address, a reflect pad not smaller than the dimension, a misaligned fp32
 * side) return DVSR_ERR_INVALID before any launch.  The sitings and DVSR_YUV_BT2020NC of the section above apply as they are.
 * depth 16 and transfer functions are not provided. */
#define DVSR_YUV16_SEMI_MSB 0     /* plane[0] = Y [h][w], plane[1] = CbCr interleaved [Hc][Wc][2]; plane[2] ignored */
#define DVSR_YUV16_PLANAR_LSB 1   /* plane[0] = Y, plane[1] = Cb [Hc][Wc], plane[2] = Cr [Hc][Wc] */
typedef struct dvsr_yuv16_desc {
  int format, depth;         /* DVSR_YUV16_*, or DVSR_YUV_FORMAT(one of them, DVSR_YUV_CHROMA_*); depth 10 or 12 */
  int h, w;                  /* the frame's own (luma) size */
  int matrix, range;         /* DVSR_YUV_BT601 / _BT709 / _BT2020NC, DVSR_YUV_LIMITED / _FULL */
  void* plane[3];
  long long row_stride[3];   /* bytes, even */
} dvsr_yuv16_desc;
int dvsr_frame_ingest_yuv16(const dvsr_yuv16_desc* sd, float* dst, int Hp, int Wp, int pad_mode, dvsr_stream_t stream);
int dvsr_frame_emit_yuv16(const float* src, int Hs, int Ws, const dvsr_yuv16_desc* dd, float lo, float hi, dvsr_stream_t stream);
int dvsr_edvr_stream_extract_frame_yuv16(const dvsr_edvr_stream* stream_plan, const float* const* params,
                                         const dvsr_yuv16_desc* fd, int pad_mode, int slot, void* cache, size_t cache_bytes,
                                         void* workspace, size_t workspace_bytes, int packed, dvsr_stream_t stream);

/* ---- SR frames at a target output size: the resampler in front of the emit functions -----------------
 * Separable antialiased bicubic: Keys' kernel with a = -0.5, half-pixel centres, the support widened by the down-scale
 * ratio -- torch.nn.functional.interpolate(x, size=(oh, ow), mode='bicubic', antialias=True, align_corners=False).
 * Per axis, n_in -> n_out:  scale = n_in / n_out;  support = 2 scale and inv = 1 / scale if scale >= 1, else 2 and 1.  Output
 * i: c = scale (i + 0.5), first = max(0, int(c - support + 0.5)), end = min(n_in, int(c + support + 0.5)), and
 * w_j = k((j - c + 0.5) inv) for j in [first, end), divided by their sum;  k(x) = ((a+2)|x| - (a+3)) x^2 + 1 for |x| < 1,
 * a (((|x| - 5)|x| + 8)|x| - 4) for 1 <= |x| < 2, 0 otherwise.  The window is cut at the edge of the image and renormalised.
 * Accepted per axis: n_in / n_out <= 4 and n_out / n_in <= 2 (at most 18 taps).
 * dvsr_frame_resize_taps: the longest window end - first of the axis.  Host code, no device call.
 * dvsr_frame_resize_table: first[n_out] and weights[n_out][taps] (HOST memory), taps >= dvsr_frame_resize_taps and <= 18;
 *   weights are computed in double, rounded to fp32 and zero-padded to taps.  Host code, no device call.
 * dvsr_frame_resize: src fp32 planar [3][Hs][Ws] (16-byte aligned, Ws % 4 == 0: the fuse tape's output), of which ONLY the
 *   top-left h x w is the image -- the padding around it is never read -- -> dst fp32 planar [3][Ho][Wo] (16-byte aligned,
 *   Wo % 4 == 0, Ho >= oh, Wo >= ow): rows 0 .. oh-1 hold the oh x ow image in columns 0 .. ow-1 and 0 in columns ow .. Wo-1,
 *   rows oh .. Ho-1 are not written.  dst is what dvsr_frame_emit / _emit_yuv / _emit_yuv16 take as src.  Columns are
 *   resampled first, then rows, in fp32.  rows / cols: the tables of h -> oh / w -> ow as dvsr_frame_resize_table fills
 *   them, copied to DEVICE memory.  The kernel clamps every index into the image: a table with other contents gives a wrong
 *   picture, never an access outside src's h x w or dst's oh x Wo.  One launch, no atomics, deterministic.
 * Bad arguments (null pointer, a size < 1, h x w or oh x ow beyond its tensor, Ws or Wo no multiple of 4, a ratio outside
 * the bounds, taps outside [1, 18] or shorter than the axis needs, a misaligned tensor or table) return DVSR_ERR_INVALID
 * before any launch. */
typedef struct dvsr_resize_axis {
  const int* first;       /* [n_out]        device memory */
  const float* weights;   /* [n_out][taps]  device memory */
  int taps;
} dvsr_resize_axis;
int dvsr_frame_resize_taps(int n_in, int n_out);
int dvsr_frame_resize_table(int n_in, int n_out, int taps, int* first, float* weights);
int dvsr_frame_resize(const float* src, int Hs, int Ws, int h, int w, float* dst, int Ho, int Wo, int oh, int ow,
                      const dvsr_resize_axis* rows, const dvsr_resize_axis* cols, dvsr_stream_t stream);

/* ---- Flip-test x4 self-ensemble: the flips in front of the network and the mean of the un-flipped outputs behind it ----
 * The reference's flipx4_forward (utils/util.py:232-254; `flip_test` of test_Vid4_REDS4_with_GT.py) runs the network on a clip
 * as it is, flipped in W, flipped in H and flipped in both, un-flips the three outputs and averages the four.
 * Both functions work on contiguous fp32 planar [planes][H][W] with W % 4 == 0 and 16-byte aligned pointers -- an ingested
 * frame, a clip (planes = B N 3), the fuse tape's output.
 * dvsr_frame_flip: dst[p][y][x] = src[p][fy(y)][fx(x)], fx(x) = W-1-x if flags & DVSR_FLIP_W (else x), fy(y) = H-1-y if
 *   flags & DVSR_FLIP_H (else y); flags = 0 is a copy.
 * dvsr_frame_flip_mean: dst[p][y][x] = (((y0[p][y][x] + yw[p][y][W-1-x]) + yh[p][H-1-y][x]) + yhw[p][H-1-y][W-1-x]) * 0.25f,
 *   the additions in exactly this order (the reference's statements), in fp32 and never contracted: the bits of the torch
 *   composition.
 * One launch each, 16-byte loads and stores only, no atomics, deterministic; every element of dst is written and nothing else.
 * dst must not be one of the sources (nor overlap one): nothing works in place.
 * Bad arguments (null pointer, planes / H / W < 1, W no multiple of 4, a misaligned pointer, flags outside 0 .. 3, dst equal
 * to a source) return DVSR_ERR_INVALID before any launch. */
#define DVSR_FLIP_W 1
#define DVSR_FLIP_H 2
int dvsr_frame_flip(const float* src, float* dst, long long planes, int H, int W, int flags, dvsr_stream_t stream);
int dvsr_frame_flip_mean(const float* y0, const float* yw, const float* yh, const float* yhw, float* dst,
                         long long planes, int H, int W, dvsr_stream_t stream);

/* ---- Frames in overlapping tiles: the tile grid, the blend weights, and the launch that stitches the SR tiles ----------
 * A frame too large for one plan is cut into tiles of ONE size, super-resolved tile by tile and blended at the seams.
 * Per axis, on the padded length n (LR pixels): n, tile multiples of 4 and >= 4, overlap a multiple of 4 with
 * 0 <= overlap <= tile / 2.  tile >= n: one tile of length n at 0.  Otherwise step = tile - overlap and the origins are
 * k step for every k step < n - tile, then n - tile (the last tile is anchored at the edge); a position is covered by at
 * most 3 tiles.  In SR pixels at scale s (L = s min(tile, n), O_k = s origin_k) tile k has at O_k <= r < O_k + L the raw
 * weight u_k(r) = min(dl, dr), dl = r - O_k + 0.5 (L for the first tile), dr = O_k + L - r - 0.5 (L for the last one), and
 * the weight w_k(r) = u_k(r) / sum_j u_j(r): a linear cross-fade in a pairwise overlap, exactly 1.0f where one tile covers.
 * dvsr_frame_stitch_origins: the number of tiles; origins[0 .. count) (HOST, LR pixels) when origins != NULL (capacity >=
 *   count).  dvsr_frame_stitch_cover: K, the largest number of tiles over one position (1 .. 3).  dvsr_frame_stitch_table:
 *   first[s n] (the first tile covering each SR position) and weights[s n][cover] (HOST memory; cover >= K and <= 3), computed
 *   in double, rounded to fp32, zero-padded; 1 <= s <= 16.  Host code, no device call.
 * dvsr_frame_stitch: tiles fp32 contiguous [ny nx][planes][Ht][Wt], tile (iy, ix) at index iy nx + ix  ->  dst fp32
 *   [planes][H][W]; Ht, Wt, H, W multiples of 4, H and planes <= 65535, every pointer 16-byte aligned.
 *     dst[p][r][c] = sum_a sum_b (wy[r][a] wx[c][b]) tile(first_y[r] + a, first_x[c] + b)[p][r - O_y][c - O_x],
 *   a outer, b inner, the product of the two weights first, then the product with the value, the accumulator starting as the
 *   first term, in fp32 and never contracted: the bits of the same loop in torch.  An entry whose row or column weight is
 *   exactly 0 is neither read nor added.  Columns go in 16-byte chunks: first_x is read at a chunk's first column and a column
 *   index is clamped chunk-wise (origins are multiples of 4, so the four columns of a chunk share their tiles).  rows / cols: the tables of the axis as dvsr_frame_stitch_table fills them and the
 *   origins in SR pixels, copied to DEVICE memory (weights 16-byte aligned); origins_y[ny] / origins_x[nx]: the same origins
 *   in HOST memory, which the call checks (0 first, H - Ht resp. W - Wt last, ascending multiples of 4, no gap).  The kernel
 *   clamps every index into `tiles` and dst: a table with other contents gives a wrong picture, never an access outside
 *   either tensor.  One launch, 16-byte loads and stores only, no atomics, deterministic; every element of dst is written once
 *   and nothing else is.  dst must not overlap tiles.
 * Bad arguments (null or misaligned pointer, ny / nx / planes < 1, a size that is no multiple of 4, cover outside 1 .. 3,
 * origins inconsistent with H, W, Ht, Wt, dst overlapping tiles) return DVSR_ERR_INVALID before any launch. */
typedef struct dvsr_stitch_axis {
  const int* first;       /* [N]         device memory; N = H (rows) or W (columns) */
  const float* weights;   /* [N][cover]  device memory */
  const int* origins;     /* [tiles]     device memory, SR pixels */
  int cover;
} dvsr_stitch_axis;
int dvsr_frame_stitch_origins(int n, int tile, int overlap, int* origins, int capacity);
int dvsr_frame_stitch_cover(int n, int tile, int overlap);
int dvsr_frame_stitch_table(int n, int tile, int overlap, int scale, int cover, int* first, float* weights);
int dvsr_frame_stitch(const float* tiles, int ny, int nx, int planes, int Ht, int Wt, float* dst, int H, int W,
                      const dvsr_stitch_axis* rows, const dvsr_stitch_axis* cols, const int* origins_y, const int* origins_x,
                      dvsr_stream_t stream);

/* ---- Down-scaling estimators MFDN / SFDN as one launch tape ------------------------------------
 * Replaces DirectKernelEstimatorVideo.forward (models/archs/LRimg_estimator.py:92-117, "MFDN":
 * Conv3d(k3)+ReplicationPad3d, ReflectionPad2d + 3x3 / 4x4-stride-2 Conv2d, Conv3d, 1x1, per-frame
 * mean subtraction / re-addition) and DirectKernelEstimator_CMS.forward (:55-67, "SFDN", x2) plus their
 * autograd backward w.r.t. the parameters -- the estimator sits inside the inner-step graph
 * (test_dynavsr.py:237-241) but its input clip is data, so no input gradient is produced.
 * x: [B][in_nc][T][H][W] fp32 for MFDN (the layout feed_data builds, LRestimator_model.py:103),
 * [B][in_nc][H][W] for SFDN; out: [B][in_nc][T][H/scale][W/scale] (SFDN: [B][in_nc][H/2][W/2]).
 * params / grad_params: host arrays of dvsr_estimator_num_params() (= 14) device pointers in
 * state-dict order conv0.weight, conv0.bias, ..., conv6.bias; gradients are overwritten.
 * Workspace protocol as for the EDVR plan (need_grad=1 before the forward whose backward follows). */
#define DVSR_ESTIMATOR_MFDN 0
#define DVSR_ESTIMATOR_SFDN 1
typedef struct dvsr_estimator_config {
  int kind;    /* DVSR_ESTIMATOR_* */
  int nf;      /* 64 in every shipped YAML */
  int in_nc;   /* 3 */
  int scale;   /* MFDN: 2 or 4; SFDN: 2 */
  int nframes; /* T (MFDN); ignored for SFDN */
} dvsr_estimator_config;
typedef struct dvsr_estimator_plan dvsr_estimator_plan;
int dvsr_estimator_plan_create(const dvsr_estimator_config* cfg, int B, int H, int W, dvsr_estimator_plan** out);
/* Per-group parameter gradients, as dvsr_edvr_plan_create_grouped: grad_params[i] = [grad_groups][numel(param i)]. */
int dvsr_estimator_plan_create_grouped(const dvsr_estimator_config* cfg, int B, int H, int W, int grad_groups,
                                       dvsr_estimator_plan** out);
/* ... with per-group weights, as dvsr_edvr_plan_create_ex. */
int dvsr_estimator_plan_create_ex(const dvsr_estimator_config* cfg, int B, int H, int W, int grad_groups, int weight_sets,
                                  dvsr_estimator_plan** out);
void dvsr_estimator_plan_destroy(dvsr_estimator_plan* plan);
int dvsr_estimator_num_params(const dvsr_estimator_plan* plan);
/* tape length: forward ops (backward = 0) or backward ops (backward = 1); a measurement aid like
 * dvsr_edvr_num_launches / dvsr_edvr_num_backward_launches */
int dvsr_estimator_num_launches(const dvsr_estimator_plan* plan, int backward);
int dvsr_estimator_plan_work(const dvsr_estimator_plan* plan, double* out9);   /* as dvsr_edvr_plan_work */
size_t dvsr_estimator_workspace_bytes(const dvsr_estimator_plan* plan, int need_grad);
int dvsr_estimator_forward(const dvsr_estimator_plan* plan, const float* const* params, const float* x, float* out,
                           void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_estimator_backward(const dvsr_estimator_plan* plan, const float* const* params, const float* x,
                            const float* grad_out, float* const* grad_params, void* workspace,
                            size_t workspace_bytes, dvsr_stream_t stream);

/* ---- Charbonnier loss (models/loss.py:19-30, the `pixel_criterion: cb` of every EDVR YAML) --------
 * loss[0] = mean(sqrt((x-y)^2 + eps)), deterministic two-stage reduction; backward writes
 * gx = grad_loss[0]/n * (x-y)/sqrt((x-y)^2+eps) (the gradient w.r.t. y is -gx). */
size_t dvsr_charbonnier_workspace_bytes(void);
int dvsr_charbonnier_forward(const float* x, const float* y, float* loss, long long n, float eps,
                             void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_charbonnier_backward(const float* x, const float* y, const float* grad_loss, float* gx, long long n,
                              float eps, dvsr_stream_t stream);
/* Per-group losses of a batch: x, y = [groups][n]; loss[g], grad_loss[g] per group; every group is reduced exactly as a
 * scalar call on its n elements would be (same partial sums, same order -> bit-identical values).  The K frames adapted
 * as one batch (dvsr_edvr_plan_create_grouped) each have their own `cri_pix(netG(SLR), LR_center)`, models/loss.py:26-30.
 * Workspace: groups * dvsr_charbonnier_workspace_bytes(). */
int dvsr_charbonnier_forward_grouped(const float* x, const float* y, float* loss, long long n, int groups, float eps,
                                     void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_charbonnier_backward_grouped(const float* x, const float* y, const float* grad_loss, float* gx, long long n,
                                      int groups, float eps, dvsr_stream_t stream);

/* ---- loss tail of the inner MAML step (test_dynavsr.py:264-274) ------------------------------------------
 * loss = cri_pix(netG(SLR), LR_center) + 10 * F.l1_loss(SLR, SLR_fixed): loss[0] = (base ? base[0] : 0) +
 * weight * mean|x - y| with `base` the pixel loss already on the device (one reduction + one 1-thread kernel instead
 * of the abs / mean / mul / add chain); backward writes gx = grad_loss[0] * weight / n * sign(x - y) (sign(0) = 0,
 * as torch's l1_loss); the gradient w.r.t. base is grad_loss itself.  Workspace: dvsr_charbonnier_workspace_bytes(). */
int dvsr_l1_tail_forward(const float* x, const float* y, const float* base, float weight, float* loss, long long n,
                         void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_l1_tail_backward(const float* x, const float* y, const float* grad_loss, float weight, float* gx, long long n,
                          dvsr_stream_t stream);
/* Per-group form, as dvsr_charbonnier_*_grouped: x, y = [groups][n]; base, loss, grad_loss = [groups]. */
int dvsr_l1_tail_forward_grouped(const float* x, const float* y, const float* base, float weight, float* loss, long long n,
                                 int groups, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_l1_tail_backward_grouped(const float* x, const float* y, const float* grad_loss, float weight, float* gx,
                                  long long n, int groups, dvsr_stream_t stream);

/* ---- region forms of the two losses (a clip padded at the bottom and right: the objective counts the frame's own pixels)
 * x, y (and gx) = [groups][planes][H][W] contiguous fp32; the region is the top-left h x w of every plane, 1 <= h <= H,
 * 1 <= w <= W; n = planes * h * w.  Grouped like *_grouped (groups = 1: the scalar loss).
 * forward:  loss[g] = mean over the region of sqrt((x-y)^2 + eps)  /  (base ? base[g] : 0) + weight * mean over it of |x-y|.
 *           The region is walked in the row-major order of the cropped tensor with the grid, stride and reduction of the
 *           functions above: the value is bit-identical to theirs on a contiguous copy of the crop.
 * backward: writes EVERY element of gx -- inside the region the formulas above with 1/n (bit-identical to them on the
 *           crop), outside exactly 0.f -- so gx may be uninitialised memory.
 * Workspace (forward): groups * dvsr_charbonnier_workspace_bytes(). */
int dvsr_charbonnier_region_forward(const float* x, const float* y, float* loss, int groups, long long planes, int H, int W,
                                    int h, int w, float eps, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_charbonnier_region_backward(const float* x, const float* y, const float* grad_loss, float* gx, int groups,
                                     long long planes, int H, int W, int h, int w, float eps, dvsr_stream_t stream);
int dvsr_l1_tail_region_forward(const float* x, const float* y, const float* base, float weight, float* loss, int groups,
                                long long planes, int H, int W, int h, int w, void* workspace, size_t workspace_bytes,
                                dvsr_stream_t stream);
int dvsr_l1_tail_region_backward(const float* x, const float* y, const float* grad_loss, float weight, float* gx, int groups,
                                 long long planes, int H, int W, int h, int w, dvsr_stream_t stream);

/* ---- op-level entries to the pipelined / small-grid conv kernels ---------------------------------------------------
 * dvsr_conv2d_forward needs no workspace and runs the un-packed kernel.  These pack the weights into a caller
 * workspace on the stream and run the geometry the whole-network plan would pick for the shape (pipelined 4-row tiles,
 * or the K-split kernel on small grids): 1x1 and 3x3, stride 1, pad ks/2; same descriptor and epilogues.  The data
 * gradient is the same kernel over the transposed, tap-mirrored pack (single plain input). */
size_t dvsr_conv2d_packed_workspace_bytes(const dvsr_conv2d_desc* d);
int dvsr_conv2d_forward_packed(const dvsr_conv2d_desc* d, void* workspace, size_t workspace_bytes, dvsr_stream_t stream);
int dvsr_conv2d_dgrad_packed(const dvsr_conv2d_desc* d, const float* gy, float* gx0, void* workspace,
                             size_t workspace_bytes, dvsr_stream_t stream);
/* Which kernel dvsr_conv2d_forward_packed runs for d (tests and tools): geo[0..3] = input channels per chunk,
 * tile rows (x 32 pixels), 32-output-channel halves per workgroup, 1 when the halo is staged by LDS-DMA
 * (conv2d_dma_kernel: 3x3 / stride 1, 16-byte aligned inputs, W % 4 == 0, channel counts % 8 == 0), 2 for the row-split
 * DMA kernel of 7x7 / 9x9 convolutions (conv2d_dmarow_kernel) -- for those sizes the packed entries exist ONLY when
 * geo[3] == 2, otherwise use dvsr_conv2d_forward / _backward.  32-channel chunks = the K-split small-grid kernel.
 * geo[3] == 3: the Winograd F(2x2, 3x3) kernel (conv2d_wino_kernel; the DMA-halo kernel's conditions and at least 16 input
 * channels; geo[1] = 4: 4x64-pixel workgroup tiles, 8: 8x32), chosen per shape by a cost model; the environment variable
 * DVSR_CONV_WINO=0 keeps the direct kernels, =2 takes it wherever it is eligible.  Same results within fp32 round-off. */
int dvsr_conv2d_packed_geometry(const dvsr_conv2d_desc* d, int geo[4]);

/* Weight / bias gradient of a single-input 3x3 stride-1 convolution with both operands rounded to bf16 on
 * v_mfma_f32_32x32x16_bf16 (fp32 accumulation and flush): what the EDVR plan runs for its weight gradients when
 * network_G.bf16_mfma = 1 (BASELINE configs[4]).  gy = gradient w.r.t. the pre-activation output; gb may be NULL.
 * Workspace: dvsr_conv2d_backward_workspace_bytes(d). */
int dvsr_conv2d_wgrad_bf16(const dvsr_conv2d_desc* d, const float* gy, float* gw, float* gb, void* workspace,
                           size_t workspace_bytes, dvsr_stream_t stream);
/* The same weight gradient at fp32 accuracy on the bf16 pipe: both operands split exactly into three bf16 pieces, six
 * partial products per fp32 product (what the plans run for 3x3 stride-1 layers; arguments as dvsr_conv2d_wgrad_bf16). */
int dvsr_conv2d_wgrad_split3(const dvsr_conv2d_desc* d, const float* gy, float* gw, float* gb, void* workspace,
                             size_t workspace_bytes, dvsr_stream_t stream);

/* Which kernel a weight gradient runs on and how it is launched: the counterpart of dvsr_conv2d_packed_geometry.  The launch
 * is the one dvsr_conv2d_wgrad_bf16 (mode 1), dvsr_conv2d_wgrad_split3 (mode 2) or the weight gradient of dvsr_conv2d_backward
 * (mode 0, with d->pad = ks / 2) makes for d's first input; of d->x0 and d->y -- standing for the gradient, which has its shape --
 * only the alignment is read (pixel_shuffle: the gradient is stored shuffled, as the EDVR plans have it).  groups >= 1: that
 * many per-group gradients.  geo = {kernel, row_split, vx, nsplit, nslot, grid x, grid y, grid z}; kernel: 0 the simple fp32
 * kernel (stride 2), 1 the pipelined fp32 kernel, 2 plain bf16, 3 / 4 / 5 the exact bf16 split with scalar staging / vector
 * staging / vector staging on eight waves; row_split = 1: one kernel row per workgroup (small pixel grids).  Launches nothing and
 * needs no device.  dvsr_conv2d_wgrad_workspace_bytes: the workspace such a launch needs (dvsr_conv2d_backward_workspace_bytes
 * is its groups = 1, pad = ks / 2 case over the wider of the two inputs). */
int dvsr_conv2d_wgrad_geometry(const dvsr_conv2d_desc* d, int mode, int groups, int geo[8]);
size_t dvsr_conv2d_wgrad_workspace_bytes(const dvsr_conv2d_desc* d, int groups);

/* ---- The DVSR_* environment switches (A/B aids and kill-switches; INTEGRATION.md lists them) ----------------
 * One table in the library states every switch's name, scope, parser and default; these queries read it and need no device.
 * Scope = when the library reads the variable: */
#define DVSR_SW_BUILD 0   /* every time a plan is built or an op-level entry chooses a geometry: part of a plan's identity */
#define DVSR_SW_PROCESS 1 /* at the switch's own first use, then kept: set it before the first call, one process per value */
#define DVSR_SW_CALL 2    /* on every call */
#define DVSR_SW_DEBUG 3   /* on every call, and consumed by the -DDVSR_CONV_TRACE build only */
int dvsr_switch_count(void);
/* Row i in [0, count): the variable's name, its scope, its value when unset and one line of documentation (static strings;
 * any pointer may be NULL). */
int dvsr_switch_info(int i, const char** name, int* scope, int* dflt, const char** doc);
/* What row i's parser makes of `text` (NULL: the variable is unset).  Does not touch the environment. */
int dvsr_switch_parse(int i, const char* text, int* value);
/* What the library itself takes switch i for now, under its scope (a PROCESS switch: this is a first use like any other). */
int dvsr_switch_value(int i, int* value);

/* ---- TOFlow backbone ops (codes/models/archs/TOF_arch.py:25-140, arch_util.py:55-79) --------
 * The convolutions of SpyNet (7x7) and of the TOFlow head (9x9, 1x1) go through dvsr_conv2d_forward / _backward
 * (ks = 7, 9, 1); the ops below are the rest of the graph.  All fp32 NCHW, HBM-bound streaming kernels.
 *
 * flow_warp (arch_util.py:55-79): out[n,c,y,x] = bilinear sample of x[n,c] at (x + flow[n,0,y,x], y + flow[n,1,y,x])
 * through F.grid_sample's align_corners=False mapping of the (size-1)-normalised grid, zeros padding.  `flow` is
 * channel-first [N,2,H,W] (the reference permutes to NHW2 first).  out_bstride / gout_bstride (0 = dense) let the
 * output be a channel slice of a wider tensor (torch.cat([ref, warped, flow]) is built in place).  Backward:
 * grad_x (zeroed here, atomics) and / or grad_flow; either may be NULL. */
int dvsr_flow_warp_forward(const float* x, const float* flow, float* out, int N, int C, int H, int W,
                           long long out_bstride, dvsr_stream_t stream);
int dvsr_flow_warp_backward(const float* x, const float* flow, const float* grad_out, float* grad_x, float* grad_flow,
                            int N, int C, int H, int W, long long gout_bstride, dvsr_stream_t stream);
/* F.avg_pool2d(x, kernel_size=2, stride=2) (TOF_arch.py:67-74); planes = N*C; output (H/2) x (W/2). */
int dvsr_avgpool2_forward(const float* x, float* y, long long planes, int H, int W, dvsr_stream_t stream);
int dvsr_avgpool2_backward(const float* grad_y, float* grad_x, long long planes, int H, int W, int accumulate,
                           dvsr_stream_t stream);
/* F.interpolate(x, size=(Ho,Wo), mode='bilinear', align_corners=True) * mul (TOF_arch.py:84-85); y_plane_stride
 * (0 = Ho*Wo) addresses a channel slice.  Backward zeroes grad_x and scatters. */
int dvsr_resize_bilinear_ac_forward(const float* x, float* y, long long planes, int H, int W, int Ho, int Wo, float mul,
                                    long long y_plane_stride, dvsr_stream_t stream);
int dvsr_resize_bilinear_ac_backward(const float* grad_y, float* grad_x, long long planes, int H, int W, int Ho, int Wo,
                                     float mul, long long gy_plane_stride, dvsr_stream_t stream);
/* F.interpolate(x, scale_factor=scale, mode='bicubic', align_corners=True): the drivers bring the (S)LR clip to the
 * output size before TOFlow (test_dynavsr.py:188-193, 245-250; train_dynavsr.py:314-320).  ATen's cubic convolution
 * (A = -0.75), clamped taps.  Backward zeroes grad_x and scatters. */
int dvsr_upsample_bicubic_ac_forward(const float* x, float* y, long long planes, int H, int W, int scale,
                                     dvsr_stream_t stream);
int dvsr_upsample_bicubic_ac_backward(const float* grad_y, float* grad_x, long long planes, int H, int W, int scale,
                                      dvsr_stream_t stream);
/* out[n,c,:] (+)= x[n,c,:] * scale[c] + shift[c]; scale / shift may be NULL (1 / 0): normalize / denormalize
 * (TOF_arch.py:13-22) and channel-slice copies; batch strides 0 = dense. */
int dvsr_channel_affine(const float* x, const float* scale, const float* shift, float* out, int N, int C, long long HW,
                        long long x_bstride, long long out_bstride, int accumulate, dvsr_stream_t stream);
/* nn.BatchNorm2d (+ the ReLU behind it, TOF_arch.py:33-42).  training != 0: batch statistics, running estimates
 * updated in place (momentum, unbiased variance); else the running estimates.  save_mean / save_rstd [C] feed the
 * backward, which takes the gradient w.r.t. the (post-ReLU) output and needs y only when relu. */
size_t dvsr_batchnorm_workspace_bytes(int C);
int dvsr_batchnorm_forward(const float* x, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float* y, float* save_mean, float* save_rstd, int N, int C, long long HW,
                           int training, float momentum, float eps, int relu, void* workspace, size_t workspace_bytes,
                           dvsr_stream_t stream);
int dvsr_batchnorm_backward(const float* x, const float* grad_y, const float* y, const float* gamma,
                            const float* save_mean, const float* save_rstd, float* grad_x, float* grad_gamma,
                            float* grad_beta, int N, int C, long long HW, int training, int relu, void* workspace,
                            size_t workspace_bytes, dvsr_stream_t stream);

/* ---- DUF backbone ops (codes/models/archs/DUF_arch.py:32-180) ------------------------------------
 * Frames are the batch axis ([B*T][C][H][W]).  Conv3d (1,3,3) / (1,1,1) are dvsr_conv2d_* over the frames; the (3,3,3)
 * Conv3d of the dense blocks (:45-58) is a 3x3 conv2d over 3C channels after this gather of frames t-1, t, t+1:
 * y[(b*To + t)][c*3 + kt] = x[(b*T + t + kt - pad_t)][c] or 0; pad_t = 1 keeps T (padding (1,1,1)), pad_t = 0 is the
 * T-reducing block (padding (0,1,1), To = T - 2).  The Conv3d weight [Cout][C][3][3][3] is that conv's
 * [Cout][3C][3][3] weight as it lies in memory.  BatchNorm3d = dvsr_batchnorm_* over N = B*T. */
int dvsr_temporal_gather3_forward(const float* x, float* y, int B, int T, int C, long long HW, int pad_t,
                                  dvsr_stream_t stream);
int dvsr_temporal_gather3_backward(const float* grad_y, float* grad_x, int B, int T, int C, long long HW, int pad_t,
                                   dvsr_stream_t stream);
/* Tail of DUF.forward (:160-176) in one kernel: Fx = softmax over the 25 taps of filter_logits [B][25*R][H][W]
 * (channel f*R + r, R = scale^2), DynamicUpsamplingFilter_3C (:86-110) of the centre frame x_center [B][3][H][W] (5x5
 * patch, zero padded), + residual [B][3R][H][W] (channel c*R + r, or 3r + c when adapt_official reorders it, :17-29),
 * F.pixel_shuffle(scale) -> out [B][3][scale*H][scale*W].  Backward: grad_logits and grad_residual are written in
 * full; grad_x_center may be NULL (the clip is data in the inner loop).  adapt_official is a bit set: bit 0 = the
 * residual's channel order above; bit 1 = `filter_logits` already holds the 25 filter TAPS, applied as given with no
 * softmax (DynamicUpsamplingFilter_3C used as a module on its own, :100-110; grad_logits is then d/d(taps)). */
int dvsr_dynamic_filter_forward(const float* x_center, const float* filter_logits, const float* residual, float* out,
                                int B, int H, int W, int scale, int adapt_official, dvsr_stream_t stream);
int dvsr_dynamic_filter_backward(const float* x_center, const float* filter_logits, const float* grad_out,
                                 float* grad_logits, float* grad_residual, float* grad_x_center, int B, int H, int W,
                                 int scale, int adapt_official, dvsr_stream_t stream);

/* ---- 3x3 convolution with very few outputs (EDVR's conv_last: 64 -> 3 at the HR size) -------------------------
 * y = act(conv3x3(x, w) + bias) [+ res], stride 1, zero padding 1, Cout <= 4; x [N][C][H][W], w [Cout][C][3][3], res / y
 * [N][Cout][H][W] (res may be NULL: EDVR_arch.py:311-312 adds the bilinear base frame here).  C = 64, Cout <= 3, W % 4 == 0
 * and 16-byte aligned tensors run as a 9 Cout-row GEMM on the fp32 matrix pipe + a shift-add; everything else on the
 * vector ALU. */
int dvsr_conv3x3_small_cout(const float* x, const float* w, const float* bias, const float* res, float* y, int N, int C, int H,
                            int W, int Cout, int act, dvsr_stream_t stream);

/* ---- two 1x1 convolutions over one input (TSA fusion) ---------------------------------------------------
 * EDVR_arch.py:183-202: fea = lrelu(fea_fusion(x)), att = lrelu(sAtt_1(x)) read the same [N][Cin][H][W] tensor (Cin = nframes *
 * nf); one pass over it produces both [N][64][H][W] outputs.  w0 / w1: [64][Cin] (the modules' [64][Cin][1][1] weights), b0 /
 * b1: [64] or NULL, act as in dvsr_conv2d_desc.  Needs Cin % 16 == 0, (H * W) % 4 == 0 and 16-byte aligned tensors; anything
 * else returns DVSR_ERR_UNSUPPORTED (the plans fall back to two dvsr_conv2d launches). */
int dvsr_conv1x1_dual(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, float* y0, float* y1,
                      int N, int Cin, int H, int W, int act, dvsr_stream_t stream);

/* ---- random patch crops of the inner step (train.maml.use_patch) -----------------------------------------
 * test_dynavsr.py:118-145 (and train_dynavsr.py:208-243) crop `num_patch` random patches out of the SLR clip and its
 * target with preprocessing.common_crop (data/meta_learner/preprocessing.py:57-85) and stack them into a batch.
 * dst[p][n][y][x] = src[n][scale*py[p] + y][scale*px[p] + x] for n < planes, 0 <= y, x < scale*edge; py / px are HOST
 * arrays of P <= 64 positions on the lowest-resolution grid (the host draws them, like the reference).  Backward
 * zeroes grad_src and adds the (overlapping) patches back with atomics. */
int dvsr_patch_gather_forward(const float* src, float* dst, const int* py, const int* px, int P, int planes, int H, int W,
                              int edge, int scale, dvsr_stream_t stream);
int dvsr_patch_gather_backward(const float* grad_dst, float* grad_src, const int* py, const int* px, int P, int planes,
                               int H, int W, int edge, int scale, dvsr_stream_t stream);

/* ---- inner-loop optimiser steps over lists of parameter tensors ------------------------------------
 * test_dynavsr.py:223-231 steps torch.optim.Adam(lr_alpha, betas) / torch.optim.SGD(lr_alpha) over the
 * ~158 tensors of netG + netE once per inner iteration; these entry points do one such step (same
 * single-tensor formulas, no amsgrad / momentum) with one launch per 48 tensors.  All arrays are HOST
 * arrays of length n_tensors; a NULL gradient or numel <= 0 skips that tensor (torch.optim skips
 * parameters whose .grad is None).  `step` is the 1-based step count of the Adam bias correction. */
int dvsr_adam_step(float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const long long* numel, int n_tensors, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, dvsr_stream_t stream);
int dvsr_sgd_step(float* const* params, const float* const* grads, const long long* numel, int n_tensors,
                  float lr, float weight_decay, dvsr_stream_t stream);
/* The per-frame deep copies of the networks (test_dynavsr.py:208 `modelcp.netG = deepcopy(model.netG)`) for a batch of
 * frames: dst[i] = [copies][numel[i]] floats, every copy = src[i].  HOST arrays of device pointers, one launch per 48
 * tensors (the framework's foreach copy with broadcast sources is one launch per tensor: 158 for netG + netE). */
int dvsr_replicate_tensors(const float* const* src, float* const* dst, const long long* numel, int n_tensors, int copies,
                           dvsr_stream_t stream);

/* ---- per-frame image metrics on the device ------------------------------------------
 * Replaces, per super-resolved frame of test_dynavsr.py:285-292 (and of the validation loops of
 * train_dynavsr.py), the device->host copy of the fp32 frame plus
 *   util.tensor2img(rlt, mode='rgb')      codes/utils/util.py:112-142   clamp to [lo,hi], rescale, x255,
 *                                                                       round half to even, uint8 HWC
 *   util.calculate_psnr(img, hr_image)    codes/utils/util.py:262-269   20 log10(255 / sqrt(mse)) over uint8
 *   util.calculate_ssim(img, hr_image)    codes/utils/util.py:271-313   11x11 Gaussian (sigma 1.5) window in
 *                                                                       float64, "valid" region, mean over
 *                                                                       pixels and channels
 * sr, gt: [C,H,W] fp32 device tensors in the network's value range (both are quantised the tensor2img way:
 * the reference's hr_image is tensor2img(GT)).  out (DEVICE, 2 doubles): out[0] = mean squared difference of
 * the two uint8 frames (exact integer sum / (C*H*W); the caller forms the PSNR, inf when 0), out[1] = mean
 * SSIM (NaN when H or W <= 10: the reference's mean of an empty map).  sr_hwc_u8 (nullable): the uint8
 * [H,W,C] image of sr for the PNG writer.  Deterministic (integer atomics + fixed-order sums). */
size_t dvsr_frame_metrics_workspace_bytes(int C, int H, int W);
int dvsr_frame_metrics(const float* sr, const float* gt, int C, int H, int W, float lo, float hi,
                       unsigned char* sr_hwc_u8, double* out, void* workspace, size_t workspace_bytes,
                       dvsr_stream_t stream);

/* ---- PSNR / SSIM of an emitted frame against its ground truth, RGB or Y ----------------------------
 * What the reference's evaluation scripts end in (test_Vid4_REDS4_with_GT*.py, calc_psnr_ssim.py): tensor2img, optionally
 * bgr2ycbcr(only_y=True) (the Vid4 protocol), util.crop_border, calculate_psnr / calculate_ssim -- for two frames that are
 * each described by a dvsr_frame_desc (any address, any pitch, their own format), in one tile launch and one fixed-order
 * finalize launch: no quantised plane in global memory, no second pass, no floating-point atomics (bit-identical from run to
 * run).  Samples of a pixel:
 *     format                                   channel DVSR_SCORE_RGB (3 samples)     channel DVSR_SCORE_Y (1 sample)
 *     DVSR_FRAME_U8_HWC_RGB / _BGR (3 | 4 B)   the bytes, in RGB order                Y8(R, G, B)
 *     DVSR_FRAME_F32_CHW (3 planes)            the quantiser of dvsr_frame_emit /     Y8 of those
 *                                              dvsr_frame_metrics on v, lo, hi
 *     DVSR_FRAME_U8_Y                          refused                                the byte
 *     DVSR_FRAME_U16_Y_MSB / _10 / _12         refused                                the d-bit level, d = depth in {10, 12}:
 *                                                                                     word >> (16 - d) (MSB), word & (2^d - 1)
 *   Y8 is rgb2ycbcr(only_y=True) of the reference (data/util.py), (65.481 R + 128.553 G + 24.966 B) / 255 + 16 rounded half to
 *   even, evaluated exactly in integers: num = 65481 R + 128553 G + 24966 B + 16 * 255000, num / 255000, an exact tie to the
 *   even level.  Over all 2^24 triples this equals both branches of the reference (uint8 image, float image) off the 194
 *   exact ties, num = 127500 mod 255000; on those the reference's float64 sum lands beside the tie and it differs from half-even
 *   by one level on 24 (RGB order) / 21 (BGR order) of them for an [H,W,3] image (31 / 26 for pixels passed as [N,3]).
 *   Both frames must reduce to ONE sample domain: 8-bit with 8-bit (depth 8), depth d with depth d.
 * Region: crop_border = k >= 0 removes k pixels on every side first (util.crop_border), H' x W' = (h - 2k) x (w - 2k) >= 1 x 1;
 *   the SSIM "valid" region is taken inside the crop.
 * out (DEVICE, 2 doubles, 8-byte aligned): out[0] = the exact integer sum of squared sample differences over the crop divided
 *   once by the number of samples; out[1] = the mean of the SSIM map (11-tap Gaussian, sigma 1.5, float64, separable) over
 *   channels and valid pixels with C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = 255 or 2^d - 1 -- NaN when H' <= 10 or W' <= 10.
 * workspace: dvsr_frame_score_workspace_bytes(channels, h, w) bytes for `channels` (3 for RGB, 1 for Y) samples per pixel
 *   of an h x w crop; the figure of the uncropped frame is enough for every crop.  8-byte aligned; need not be initialised.
 * Bad arguments (null pointer, sizes that differ, unknown format / channel / depth, a domain mismatch, RGB on a Y plane, a crop
 * that leaves nothing, a stride shorter than a row, a pixel stride the format does not have, a misaligned fp32 frame, an odd
 * address or stride of a 16-bit plane, a misaligned out) return DVSR_ERR_INVALID, a short workspace DVSR_ERR_WORKSPACE, before
 * any launch. */
#define DVSR_SCORE_RGB 0
#define DVSR_SCORE_Y 1
typedef struct dvsr_score_args {
  int channel;            /* DVSR_SCORE_RGB | DVSR_SCORE_Y */
  int crop_border, depth; /* depth 8, 10 or 12 */
  float lo, hi;           /* range of an F32_CHW side */
} dvsr_score_args;
size_t dvsr_frame_score_workspace_bytes(int channels, int h, int w);
int dvsr_frame_score(const void* a, const dvsr_frame_desc* da, const void* b, const dvsr_frame_desc* db,
                     const dvsr_score_args* args, double* out /* [2], 8-byte aligned device memory */, void* workspace,
                     size_t workspace_bytes, dvsr_stream_t stream);

/* ---- synthetic degradation on the device -------------------------------------------
 * Replaces the tensor part of Degradation.apply (codes/data/random_kernel_generator.py:84-130):
 *   img = ReflectionPad2d(K // 2)(img);  lr = conv2d(img, kernel.repeat(3,1,1,1), groups=3, stride=scale)
 * for a clip img [N,C,H,W] (N frames) -> out [N,C,Ho,Wo], Ho = (H + 2 (K//2) - K) / scale + 1.
 * kernels: [n_kernels,K,K] fp32 on the device, already centre-of-mass shifted (kernel_shift :51-76 stays on
 * the host: a 27 x 27 spline shift).  n_kernels = 1: one kernel for every frame (:91-103); otherwise frame i
 * uses kernel (i + kernel_offset) mod n_kernels (:104-122: offset 0 for N = n_kernels, -1 for N = n_kernels + 2).
 * quantise != 0 fuses vsrbase.py:185 `mul(255).clamp(0, 255).round().div(255)` into the store. */
int dvsr_degrade_apply(const float* img, const float* kernels, float* out, int N, int C, int H, int W, int K,
                       int scale, int n_kernels, int kernel_offset, int quantise, dvsr_stream_t stream);

/* ---- a ground-truth frame degraded as it arrives --------------------------------------------------
 * What test_dynavsr.py does with `degradation_mode: set | preset` to every frame of a ground-truth video -- read it, modcrop
 * it to a multiple of the scale (data/util.py:302), blur and sub-sample it, quantise the result to 8 bits -- for a frame in
 * the form a decoder delivers it, in one launch and without an fp32 copy of the HR frame:
 *   src / sd   one HR frame as dvsr_frame_ingest takes it: DVSR_FRAME_F32_CHW, DVSR_FRAME_U8_HWC_RGB or _BGR, at any address,
 *              pitch and pixel stride 3 or 4.  Only its top-left Hc x Wc is read, Hc = h - h % scale, Wc = w - w % scale.
 *   kernel     ONE centre-of-mass-shifted K x K fp32 kernel on the device; K <= 33, scale <= 4 and a reflection pad
 *              K / 2 < Hc, Wc: the limits of dvsr_degrade_apply.
 *   dst        fp32 planar RGB [3][h_lr][w_lr], row and plane strides in FLOATS, 4-byte aligned;
 *              h_lr = (Hc + 2 (K / 2) - K) / scale + 1, w_lr likewise.
 * The values are bit-identical to dvsr_degrade_apply(.., quantise) on the contiguous [1,3,Hc,Wc] crop of dvsr_frame_ingest's
 * output for the same frame: the two kernels of dvsr_degrade_apply read their input patch through a source policy (fp32 planes
 * by stride, or interleaved bytes by stride and channel as v / 255.0f, a true division) and everything behind it -- the choice
 * of the kernel by (scale, ceil(K / scale)) and DVSR_DEGRADE_GENERIC, the order of the taps, fmaf from an accumulator of 0, the
 * quantiser rintf(fminf(fmaxf(acc * 255, 0), 255)) / 255 -- is the same code.
 * Bad arguments return before any launch: a null pointer, an unknown format, a pixel stride outside {3,4}, a row stride shorter
 * than a row, Hc or Wc < 1, a pad not smaller than the crop, a destination stride shorter than w_lr (or planes that overlap), a
 * misaligned fp32 side: DVSR_ERR_INVALID; K or scale out of range: DVSR_ERR_UNSUPPORTED. */
int dvsr_frame_degrade(const void* src, const dvsr_frame_desc* sd, const float* kernel, int K, int scale, float* dst,
                       long long dst_row_stride, long long dst_plane_stride, int quantise, dvsr_stream_t stream);

/* ---- MATLAB's imresize(img, scale, 'bicubic') of a frame as it arrives ----------------------------------
 * The BI degradation of the SR literature (imresize(hr, 1 / s), antialiased) and the "Bicubic" row of its tables
 * (imresize(lr, s)): codes/data/util.py:323-524 of the reference (calculate_weights_indices, imresize, imresize_np).
 * Per axis, n_in -> n_out = ceil(n_in num / den), scale = num / den out of {1/2, 1/3, 1/4, 2/1, 3/1, 4/1}, in double:
 * kw = 4, or 4 / scale when scale < 1 and antialias != 0 (the reference's `antialiasing`);  P = ceil(kw) + 2 taps.  Output i:
 * u = (i + 1) / scale + 0.5 (1 - 1 / scale), left = floor(u - kw / 2); tap t reads the 1-based sample left + t with weight
 * c(u - left - t), or scale c((u - left - t) scale) when kw was widened, divided by the sum of the P weights;
 * c(x) = 1.5 |x|^3 - 2.5 |x|^2 + 1 for |x| <= 1, -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2 for 1 < |x| <= 2, 0 otherwise.  A 0-based
 * index outside [0, n_in) is folded back by MATLAB's periodic symmetric rule (-k -> k - 1, n_in - 1 + k -> n_in - k, period
 * 2 n_in) and its weight added, in tap order, to the tap it lands on; the taps with a non-zero weight are then one contiguous
 * window [first, first + len), len <= 16 (1/4), 11 (1/3), 8 (1/2), 4 (up-scaling).  Any n_in >= 1 is accepted (the reference
 * raises for 2 <= n_in <= 6 at 1/4, 2 .. 5 at 1/3, 2 .. 3 at 1/2, where its symmetric copy is longer than the image).
 * dvsr_frame_imresize_taps: the longest window of the axis; *n_out (may be null) receives n_out.  Host code, no device call.
 * dvsr_frame_imresize_table: first[n_out] and weights[n_out][taps] (HOST memory), taps >= dvsr_frame_imresize_taps and <= 18;
 *   the folded weights rounded to fp32 and zero-padded to taps.  Host code, no device call.
 * dvsr_frame_imresize: one launch per frame.
 *   src / sd   one frame as dvsr_frame_degrade takes it: DVSR_FRAME_F32_CHW, DVSR_FRAME_U8_HWC_RGB or _BGR, at any address,
 *              pitch and pixel stride 3 or 4; bytes become v / 255.0f, dvsr_frame_ingest's bits.  ONLY its top-left h x w crop
 *              is read (h <= sd->h, w <= sd->w: the reference's modcrop at no cost).
 *   dst        fp32 planar RGB [3][oh][ow], row and plane strides in FLOATS, 4-byte aligned; oh, ow must be the definition's
 *              n_out of h and w.  Rows outside oh and columns outside ow are not written.  quantise != 0 stores
 *              rintf(fminf(fmaxf(255 y, 0), 255)) / 255, the quantiser of dvsr_frame_degrade (round half to even).
 *   rows / cols  the tables of h and w as dvsr_frame_imresize_table fills them, copied to DEVICE memory.  The kernel clamps
 *              every index: a table with other contents gives a wrong picture, never an access outside the crop or oh x ow.
 *   Columns are resampled first, then rows, in fp32 (fmaf in tap order from an accumulator of 0).  No atomics, deterministic.
 * Bad arguments return before any launch: a null pointer, an unknown format, a pixel stride outside {3,4}, a row stride shorter
 * than a row, a crop beyond the frame, oh / ow that are not the definition's, taps outside [longest window, 18], a destination
 * stride shorter than ow (or planes that overlap), a misaligned fp32 side or table: DVSR_ERR_INVALID; a scale outside the six:
 * DVSR_ERR_UNSUPPORTED.  Not provided: other scales, different scales per axis, MATLAB's round-half-away uint8 output, kernels
 * other than the cubic, a YCbCr source. */
int dvsr_frame_imresize_taps(int n_in, int num, int den, int antialias, int* n_out);
int dvsr_frame_imresize_table(int n_in, int num, int den, int antialias, int taps, int* first, float* weights);
int dvsr_frame_imresize(const void* src, const dvsr_frame_desc* sd, int h, int w, int num, int den, int antialias, float* dst,
                        long long dst_row_stride, long long dst_plane_stride, int oh, int ow, const dvsr_resize_axis* rows,
                        const dvsr_resize_axis* cols, int quantise, dvsr_stream_t stream);

/* ---- a batch of meta-training tasks cut from frames on the device ----------------------------------------
 * What VSRBase.__getitem__ (codes/data/meta_learner/vsrbase.py:135-198) does per task on the CPU -- crop N frames, blur and
 * sub-sample them with one kernel, quantise, blur again, flip all three clips alike -- for a whole batch in a constant number
 * of launches.  A batch is a table of n items (one per frame of every task):
 *   src           the crop's top-left sample (channel 0 as stored), on the device, inside a frame as it was decoded
 *   row_stride    bytes (U8 HWC) or floats (F32 CHW);  plane_stride  floats, F32 CHW only
 *   kernel        index into kernels[n_kernels][K][K] (dvsr_task_gather ignores it)
 *   flags         on the STORE side: DVSR_FLIP_W | DVSR_FLIP_H | DVSR_TASK_TRANSPOSE
 * `items` is the table in host memory: the entry reads it during the call only and validates every row before anything is
 * launched.  `items_dev` is the caller's copy of the same bytes on the device (8-byte aligned), which the kernel reads; it must
 * stay as it is until the launch has run.  The library allocates nothing, copies nothing and never synchronises.  format is
 * DVSR_FRAME_F32_CHW, DVSR_FRAME_U8_HWC_RGB or _BGR and pixel_stride 3 or 4 (bytes only); both hold for the whole launch, as
 * does the crop H x W.
 * dvsr_task_degrade: item i, plane c of dst [n,3,Ho,Wo] (contiguous) is what dvsr_degrade_apply gives for that crop with
 *   kernels[items[i].kernel] -- ReflectionPad2d(K / 2), stride `scale`, no modcrop, Ho = (H + 2 (K / 2) - K) / scale + 1, Wo
 *   likewise, the same choice of kernel by (scale, ceil(K / scale)) and DVSR_DEGRADE_GENERIC, the same quantiser as an option,
 *   bit for bit -- stored through the item's flags: with r that result and f[y][x] = r[fy(y)][fx(x)] (fx, fy as in
 *   dvsr_frame_flip), dst[y][x] = f[y][x], or f[x][y] under DVSR_TASK_TRANSPOSE.  That is the order of the reference's augment
 *   (hflip, vflip, then the permute: preprocessing.py:209-237), applied where the reference applies it: AFTER the degradation (a
 *   flipped input through an unflipped, centre-of-mass-shifted kernel is a different image).
 * dvsr_task_gather: the same store with no blur, dst [n,3,H,W]: bytes as v / 255.0f (dvsr_frame_ingest's bits), fp32 copied.
 * Bad arguments return before any launch: a null pointer (a null items[i].src among them), n < 1, a format outside the three, a
 * pixel stride outside {3,4} for bytes, a pad K / 2 not smaller than the crop, a kernel index outside [0, n_kernels), flags
 * outside 0 .. 7, DVSR_TASK_TRANSPOSE with Ho != Wo (degrade) or H != W (gather), a row stride shorter than a crop row (or a
 * plane stride shorter than the crop's plane), a misaligned fp32 source, dst, kernels or table: DVSR_ERR_INVALID; 3 n > 65535, K
 * or scale out of range: DVSR_ERR_UNSUPPORTED. */
#define DVSR_TASK_TRANSPOSE 4
typedef struct dvsr_task_frame {
  const void* src;
  long long row_stride;
  long long plane_stride;
  int kernel;
  int flags;
} dvsr_task_frame;
int dvsr_task_degrade(const dvsr_task_frame* items, const dvsr_task_frame* items_dev, int n, int format, int pixel_stride,
                      int H, int W, const float* kernels, int n_kernels, int K, int scale, float* dst, int quantise,
                      dvsr_stream_t stream);
int dvsr_task_gather(const dvsr_task_frame* items, const dvsr_task_frame* items_dev, int n, int format, int pixel_stride, int H,
                     int W, float* dst, dvsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNAVSR_HIP_H_ */
