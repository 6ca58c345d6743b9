// Internal C++ launch API shared by the C-ABI wrappers and the EDVR engine.
#pragma once
#include "../../include/dynavsr_hip.h"
#include "common.h"
#include "switches.h"

namespace dvsr {

// Extra modes of the conv kernel used by backward-data (dgrad) launches.
struct ConvExtra {
  int wt = 0;                  // 1: weights read as the transposed, tap-mirrored view (dgrad)
  int w_ctot = 0, w_coff = 0;  // wt=1: original conv's total input channels / channel offset of this input
  int in_ps = 0;               // input is stored pixel-shuffled (gradient of a PixelShuffle(2) output)
  int in_dil = 0, Hs = 0, Ws = 0;  // input is the zero-dilated view of a [N][c0][Hs][Ws] tensor
  int accum = 0;               // y += result
  const float* gmask = nullptr;  // dgrad: multiply by act'(gmask) (fused activation backward of the producer)
  int gmask_act = 0;
  // per-sample weight sets: batch item n takes the packed weights at + (n / wdiv) * w_gs floats, the bias at + (n / wdiv) * b_gs
  int wdiv = 1; long long w_gs = 0; int b_gs = 0;
};
int conv2d_run(const dvsr_conv2d_desc& d, const ConvExtra& ex, hipStream_t st);

int mdcn_forward_run(const float* x, const float* off, long long off_bs, const float* msk,
                     long long msk_bs, int mask_logit, const float* w, const float* b, float* out,
                     int N, int C, int H, int W, int Cout, int kh, int kw, int stride, int pad,
                     int dil, int groups, int dg, int act, hipStream_t st);

// conv2d_v2.hip: pipelined kernel over pre-packed weights
// The kernel family a packed convolution launches on.  The values are ABI: dvsr_conv2d_packed_geometry writes them to geo[3].
enum class ConvKernel : int {
  REG = 0,        // register-staged halo (conv2d_pipe_kernel; with 32-channel chunks of a 3x3: the K-split small-grid kernel)
  DMA_HALO = 1,   // halo by LDS-DMA (conv2d_dma_kernel): plain pad-1 3x3 inputs on a 16-byte column grid, whole 8-channel chunks
  ROW_SPLIT = 2,  // row-split 7x7 / 9x9 (conv2d_dmarow_kernel)
  WINO_F2 = 3,    // Winograd F(2x2, 3x3) on the fp32 pipe (conv2d_wino.hip; th = 4: 4x64-pixel tiles, th = 8: 8x32)
  WINO_F2_BF16 = 4,  // the same on the bf16 pipe, exact 3-way operand split (conv2d_wino3.hip / conv2d_wino4.hip; also th = 16: 16x16)
  WINO_F4 = 5,    // Winograd F(4x4, 3x3) on the bf16 pipe (conv2d_wino5.hip; th = 8: 8x64-pixel workgroup tiles, th = 16: 16x32)
};
// The layout of a weight pack: the ConvKernel values (a pack is made for the kernel that reads it) plus the DCN split's own.
enum class PackLayout : int {
  INTERLEAVED = 0,   // channel c = 2kk + hi of the chunk (register-staged halo image)
  DMA_ORDER = 1,     // 4 consecutive channels per lane half (the planar DMA-staged halo image)
  ROW_SPLIT = 2,     // DMA_ORDER; the taps of a kernel row are contiguous anyway
  WINO_F2 = 3,       // Winograd-transformed image (conv2d_wino.hip)
  WINO_F2_BF16 = 4,  // the same as three bf16 pieces (conv2d_wino3.hip)
  WINO_F4 = 5,       // the F(4x4, 3x3) image of conv2d_wino5.hip
  DCN_SPLIT = 6,     // three bf16 pieces of the deformable conv's weights (mdcn_split.hip)
};
constexpr PackLayout pack_layout(ConvKernel k) { return static_cast<PackLayout>(static_cast<int>(k)); }
// What the kernels have in common, stated once:
constexpr bool is_winograd(ConvKernel k) { return k == ConvKernel::WINO_F2 || k == ConvKernel::WINO_F2_BF16 || k == ConvKernel::WINO_F4; }
constexpr bool on_bf16_split(ConvKernel k) { return k == ConvKernel::WINO_F2_BF16 || k == ConvKernel::WINO_F4; }   // six bf16 products per fp32 one
// (3x3 / s1 / pad 1 over plain 16-byte aligned inputs, W % 4 == 0, whole 8-channel chunks: conv2d_packed_prepare)
constexpr bool needs_dma_halo_inputs(ConvKernel k) { return k == ConvKernel::DMA_HALO || is_winograd(k); }
// fp32 products per product of the direct sum: F(2x2, 3x3) does 16 multiplies per 2x2 outputs instead of 36, F(4x4, 3x3) 36 per
// 4x4 outputs instead of 144
constexpr double multiplies_per_output_ratio(ConvKernel k) { return k == ConvKernel::WINO_F4 ? 0.25 : (is_winograd(k) ? 16.0 / 36.0 : 1.0); }
constexpr const char* kernel_tag(ConvKernel k) {   // dvsr_edvr_op_info
  return k == ConvKernel::WINO_F4 ? "w5" : (k == ConvKernel::WINO_F2_BF16 ? "w3" : (k == ConvKernel::WINO_F2 ? "w" : (k == ConvKernel::REG ? "" : "d")));
}
// layouts written by a pack kernel of their own (pack_weights_wino*_kernel, pack_weights_dcn3_kernel), not by pack_weights_kernel
// (the enum lists those last; one signed compare in pack_weights_kernel, as before the layouts had names)
constexpr bool has_own_pack_kernel(PackLayout l) { return static_cast<int>(l) >= static_cast<int>(PackLayout::WINO_F2); }

struct PackEntry {
  const float* w; float* P;
  // wt = 1: w is read as the transposed, tap-mirrored view of a [w_ctot][..] tensor at output-channel offset w_coff (dgrad);
  // wt = 0 with w_ctot > 0 (PackLayout::WINO_F4 only): the input channels [w_coff, w_coff + Ctot) of a [Cout][w_ctot][ks][ks] one
  int Cout, Ctot, KK, CC, wt, w_ctot, w_coff, ncb, nchunks, pch;
  int bf = 0;  // 1: bf16 image for the bf16 MFMA kernel (pch still counts fp32-sized slots)
  PackLayout layout = PackLayout::INTERLEAVED;
};
struct PackTable {
  int n;
  PackEntry e[48];
};
int pack_weights_run(const PackTable& t, hipStream_t st);
// channels per chunk, tile rows (x32 px), 32-cout halves per workgroup, bf16 mode (1 plain, 2 exact 3-way split), kernel family
struct ConvGeo { int cc, th, mt; int bf = 0; ConvKernel kernel = ConvKernel::REG; };
// What a launch's tensors let conv2_choose pick, beyond the register-staged kernel that takes everything:
enum ConvAllow : int {
  ALLOW_NONE = 0,
  ALLOW_KSPLIT = 1,    // the K-split small-grid kernel (plain inputs, explicit pad of 1, 32-channel chunks)
  ALLOW_DMA_HALO = 2,  // the DMA-halo / row-split kernels (needs_dma_halo_inputs)
  ALLOW_WINO = 4,      // the Winograd F(2x2) kernels: ALLOW_DMA_HALO's conditions + an epilogue they implement (plain or PixelShuffle(2) stores)
  ALLOW_WINO_F4 = 8,   // the F(4x4) kernel: ALLOW_WINO's + a forward epilogue (no accumulate / gradient mask)
  ALLOW_SHARED_DEVICE = 16,  // the launch shares the device with other streams' kernels (clips in flight side by side): between
                             // one-round Winograd grids the smaller occupied CU-time wins, not the shorter launch
  ALLOW_ONLY_F4 = 32,  // the launch needs what the F(4x4) kernel alone implements (the pre-activation addend, a pack of a slice of
                       // the input channels): F(4x4) wherever it is eligible, whatever the cost model says; the caller checks
};
constexpr ConvAllow operator|(ConvAllow a, ConvAllow b) { return static_cast<ConvAllow>(static_cast<int>(a) | static_cast<int>(b)); }
constexpr ConvAllow without(ConvAllow a, ConvAllow b) { return static_cast<ConvAllow>(static_cast<int>(a) & ~static_cast<int>(b)); }
ConvGeo conv2_choose(int ks, int stride, int N, int Ho, int Wo, int Cout, int Ctot, ConvAllow allow = ALLOW_KSPLIT);
// THE rule for a weight pack: its floats, and the table entry that makes pack_weights_run write it at P.  (cc, bf, layout) is
// what of a geometry shapes its pack; the DCN packs have no ConvGeo and say it directly.
size_t conv2_pack_floats(int ks, int Cout, int Ctot, int cc, int bf, PackLayout layout);
PackEntry conv2_pack_entry(const float* w, float* P, int ks, int Cout, int Ctot, int cc, int bf, PackLayout layout, int wt = 0,
                           int w_ctot = 0, int w_coff = 0);
inline size_t conv2_pack_floats(int ks, int Cout, int Ctot, const ConvGeo& g) {
  return conv2_pack_floats(ks, Cout, Ctot, g.cc, g.bf, pack_layout(g.kernel));
}
inline PackEntry conv2_pack_entry(const float* w, float* P, int ks, int Cout, int Ctot, const ConvGeo& g, int wt = 0, int w_ctot = 0,
                                  int w_coff = 0) {
  return conv2_pack_entry(w, P, ks, Cout, Ctot, g.cc, g.bf, pack_layout(g.kernel), wt, w_ctot, w_coff);
}
// Occupied CU-time of a launch on the F(4x4) kernel as conv2_choose models it: workgroups x (chunks x cycles + fixed cycles)
double conv2_f4_occupied_cycles(int N, int Ho, int Wo, int Cout, int Ctot, int th);
int pack_weights_wino_run(const PackTable& t, hipStream_t st);   // conv2d_wino.hip: PackLayout::WINO_F2 entries
int pack_weights_wino3_run(const PackTable& t, hipStream_t st);  // conv2d_wino3.hip: PackLayout::WINO_F2_BF16 entries
int pack_weights_wino5_run(const PackTable& t, hipStream_t st);  // conv2d_wino5.hip: PackLayout::WINO_F4 entries
int conv2d_packed_run(const dvsr_conv2d_desc& d, const float* wp, const ConvExtra& ex, const ConvGeo& geo,
                      hipStream_t st);

// conv1x1_dual.hip: two 1x1 convolutions (64 outputs each) over one input in one pass; x [N][Cin][HW], w [64][Cin]
bool conv1x1_dual_ok(const float* x, const float* w0, const float* w1, const float* y0, const float* y1, int Cin, long long HW);
int conv1x1_dual_run(const float* x, const float* w0, const float* b0, const float* w1, const float* b1, float* y0, float* y1,
                     int N, int Cin, int HW, int act, hipStream_t st, int wdiv = 1, long long w_gs = 0, int b_gs = 0);
int conv3x3_small_cout_run(const float* x, const float* w, const float* bias, const float* res, float* y, int N,
                           int C, int H, int W, int Cout, int act, hipStream_t st, int wdiv = 1, long long w_gs = 0,
                           int b_gs = 0);

// Slot reduction of a weight gradient (one entry at once, or deferred: conv2d_wgrad_run(..., defer = &entry) + wgrad_reduce_batch)
struct WgradReduceEntry {
  float* partial; float* dbp; float* dW; float* db;
  int nslot, KK, OP, CP, Cout, Cin, Ctot, c_off;
  // per-group gradients: group g reads the slots [g * nslot, (g + 1) * nslot) and writes dW + g * dW_gs, db + g * db_gs
  int ngroups = 1;
  long long dW_gs = 0, db_gs = 0;
};
constexpr int WGRAD_REDUCE_BATCH = 44;  // entries per launch (kernel-argument limit: 44 x 88 B < 4 KB)
struct WgradReduceTable {
  int n;
  WgradReduceEntry e[WGRAD_REDUCE_BATCH];
};
int wgrad_reduce_batch(const WgradReduceEntry* entries, int n, hipStream_t st, int blocks = 96);   // blocks: per entry and group
// One weight-gradient launch: dW[:, c_off:c_off+Cin, :, :] of a [Cout][Ctot][ks][ks] gradient (and db when non-null) from
// x, one input of the conv ([N/x_bdiv][Cin][H][W], batch stride x_bs or dense), and gy, the gradient of the conv's
// pre-activation output (gy_ps: stored pixel-shuffled).
struct WgradDesc {
  const float* x = nullptr; long long x_bs = 0; int x_bdiv = 1;
  const float* gy = nullptr; int gy_ps = 0;
  float* dW = nullptr; float* db = nullptr;
  int N = 0, Cin = 0, H = 0, W = 0, Cout = 0, Ctot = 0, c_off = 0, ks = 0, stride = 1, pad = -1;   // pad < 0: ks / 2
  // groups > 1: one gradient per group of N / groups consecutive batch items, written to dW + g * dW_gs (db + g * db_gs)
  int groups = 1; long long dW_gs = 0, db_gs = 0;
  int mode = 0;   // operands asked for: 0 fp32, 1 bf16, 2 the exact 3-way bf16 split (3x3 stride 1, split also 2x2; fp32 otherwise)
};
// The kernel a weight gradient launches on.  The values are ABI: dvsr_conv2d_wgrad_geometry writes them to geo[0].
enum class WgradKernel : int {
  SIMPLE = 0,        // conv2d_wgrad_kernel: stride 2
  PIPE = 1,          // conv2d_wgrad_pipe_kernel: the pipelined fp32 kernel, all taps or one kernel row per workgroup
  BF16 = 2,          // conv2d_wgrad_bf16_kernel: operands rounded to bf16
  SPLIT_SCALAR = 3,  // conv2d_wgrad_split3_kernel: the exact split, scalar staging
  SPLIT_VECTOR = 4,  // conv2d_wgrad_split3v_kernel: vector staging, all taps or one kernel row per workgroup
  SPLIT_WAVE8 = 5,   // conv2d_wgrad_split3w_kernel: vector staging, eight waves
};
constexpr bool on_bf16_pipe(WgradKernel k) { return k >= WgradKernel::BF16; }   // v_mfma_f32_*_bf16; the others v_mfma_f32_32x32x2_f32
constexpr bool on_bf16_split(WgradKernel k) { return k >= WgradKernel::SPLIT_SCALAR; }   // six bf16 products per fp32 one
struct WgradGeo {
  WgradKernel kernel = WgradKernel::PIPE;
  int row_split = 0;    // one kernel row per workgroup (ks times the workgroups): what the rule picks for SMALL pixel grids
  int vx = 0;           // WgradK::vx
  int nsplit = 1, nslot = 1;   // pixel splits / flush slots, per group
  dim3 grid; int block = 256;
};
// THE rule: which kernel a weight gradient runs on and how it is launched (conv2d_wgrad.hip).  Host arithmetic only: no
// HIP call, and of the pointers it reads the alignment alone.
WgradGeo conv2d_wgrad_choose(const WgradDesc& d);
bool wgrad_split3_default();   // DVSR_WGRAD_SPLIT3: plans ask for mode 2
size_t conv2d_wgrad_workspace_bytes(const WgradDesc& d);   // the slot regions at the most slots the rule gives this shape
// scratch_is_zero: the slot regions hold zeros (a reduce leaves them so); defer: the caller reduces a batch of layers later
// (wgrad_reduce_batch) and `ws` stays untouched until then
int conv2d_wgrad_run(const WgradDesc& d, void* ws, size_t ws_bytes, hipStream_t st, int scratch_is_zero = 0,
                     WgradReduceEntry* defer = nullptr);
size_t mdcn_backward_workspace_bytes(int N, int C, int H, int W, int Cout, int stride, int pad, int dil, int groups = 1);
int mdcn_backward_run(const float* x, const float* off, long long off_bs, const float* msk, long long msk_bs,
                      int mask_logit, const float* w, const float* gout, float* gx, float* goff,
                      long long goff_bs, float* gmsk, long long gmsk_bs, float* gw, float* gb, int N, int C,
                      int H, int W, int Cout, int stride, int pad, int dil, int dg, void* ws,
                      size_t ws_bytes, hipStream_t st, int groups = 1, long long gw_gs = 0, long long gb_gs = 0,
                      long long w_gs = 0);  // w_gs != 0: group g of the batch convolves with w + g * w_gs (per-sample weights)

// layout: the one `wp` is in -- INTERLEAVED the fp32 conv pack (pack_weights_kernel, 8-channel chunks), DCN_SPLIT the three bf16
// pieces of mdcn_split.hip; whoever makes the pack asks mdcn_pack_layout(W) and hands the answer back here.
int mdcn_forward_packed_run(const float* x, const float* off, long long off_bs, const float* msk,
                            long long msk_bs, int mask_logit, const float* wp, const float* b, float* out,
                            int N, int C, int H, int W, int Cout, int dg, int act, hipStream_t st, int wdiv = 1,
                            long long w_gs = 0, int b_gs = 0, PackLayout layout = PackLayout::INTERLEAVED);
int mdcn_fwd_variant();      // DVSR_DCN_FWD: 3 split (default), 0 dma, 2 reg
int mdcn_pack_floats();      // fp32-sized slots per (64-cout block, 8-channel chunk) of a PackLayout::DCN_SPLIT pack
PackLayout mdcn_pack_layout(int W);   // PackEntry::layout of a DCN weight pack for images of width W
int pack_weights_dcn3_run(const PackTable& t, hipStream_t st);   // mdcn_split.hip: PackLayout::DCN_SPLIT entries

struct DcnK2 {
  const float* x; const float* off; const float* msk; const float* wp; const float* bias; float* out;
  long long off_bstride, msk_bstride;
  int mask_logit;
  int N, C, H, W, Cout, dg, act;
  int tiles_x, tiles_y, ntiles, ncb, nchunks;
  int wdiv = 1; long long w_gs = 0; int b_gs = 0;   // per-sample weight sets (common.h: wset_ptr)
#ifdef DVSR_CONV_TRACE
  long long* trace;  // debug build only (tools/dcn_trace.py): 64 cycle stamps per workgroup
#endif
};
int mdcn_fwd_split_launch(const DcnK2& k, int grid, int mask_logit, hipStream_t st);   // mdcn_split.hip

// misc.hip
int upsample_bilinear_fwd(const float* x, float* y, size_t planes, int H, int W, int S, float mul,
                          hipStream_t st);
int upsample_bilinear_bwd(const float* gy, float* gx, size_t planes, int H, int W, int S, float mul,
                          int accumulate, hipStream_t st);
int pool3s2_fwd(const float* x, float* ymax, float* yavg, size_t planes, int H, int W, hipStream_t st);
int pool3s2_bwd(const float* x, const float* gmax, const float* gavg, float* gx, size_t planes,
                int H, int W, int accumulate, hipStream_t st);
int reduce_frames(float* dst, long long dst_bs, const float* src, int B, int cnt, size_t per,
                  int accumulate, hipStream_t st);
int tsa_gate_fwd(const float* emb, const float* emb_ref, const float* aligned, float* cor,
                 float* gated, int B, int N, int C, size_t HW, hipStream_t st);
int tsa_gate_bwd(const float* emb, const float* emb_ref, const float* aligned, const float* cor,
                 const float* g_gated, float* g_emb, float* g_emb_ref, float* g_aligned, int B,
                 int N, int C, size_t HW, hipStream_t st, float* gdot_scratch = nullptr);
int tsa_blend_fwd(const float* fea, const float* att, const float* add, float* out, size_t n,
                  hipStream_t st);
int tsa_blend_bwd(const float* fea, const float* att, const float* g, float* g_fea, float* g_att_io,
                  size_t n, int accumulate, hipStream_t st);
int add_inplace(float* dst, const float* src, size_t n, hipStream_t st);
int add_out(float* y, const float* a, const float* b, size_t n, hipStream_t st);
int act_bwd_inplace(float* g, const float* y, size_t n, int act, hipStream_t st);

// stream_gather.hip: the L1 / L2 / L3 features of the `nframes` cache slots `slots` (host array, passed to the kernel by
// value) -> dst[l][f][level_floats[l]]; slot s starts at cache + s * slot_floats, its level l at + src_off[l]
int stream_gather_run(const float* cache, size_t slot_floats, const size_t src_off[3], float* const dst[3],
                      const size_t level_floats[3], int nframes, const int* slots, hipStream_t st);

// side_stream.hip: the weight-gradient side stream to use beside launch stream `st`, out of a small per-device pool: the first
// that a probe finds running concurrently with it (cached).  nullptr: none overlaps.  *known = false: the probe could not run.
hipStream_t side_stream_for(hipStream_t st, bool* known = nullptr);

// frame_io.hip: a source frame (any address / pitch, h x w) -> fp32 planar [3][Hp][Wp].  _check validates everything and
// launches nothing (a caller with more launches ahead checks first); _launch expects checked arguments.
int frame_ingest_check(const char* what, const void* src, const dvsr_frame_desc* sd, const float* dst, int Hp, int Wp,
                       int pad_mode);
int frame_ingest_launch(const void* src, const dvsr_frame_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st);
// the descriptor's own part of that check (null, format, 1 <= h <= Ht, 1 <= w <= Wt, strides, fp32 alignment); dvsr_frame_degrade
// (degrade.hip) reads a source frame through it too
int frame_desc_check(const char* what, const void* ptr, const dvsr_frame_desc* d, int Ht, int Wt, bool emit);

// frame_rgb.hip: 16-bit interleaved RGB / BGR and planar integer RGB / GBR (DVSR_FRAME_U16_HWC_* / _U8_CHW_* / _U16_CHW_*), which
// dvsr_frame_ingest / _emit / _luma_sad / _score take beside the formats above and nothing else does.  frame_rgb_format decodes a
// format value (false: not one of these; an unknown depth leaves depth = 0); frame_rgb_check is frame_desc_check for them.
struct RgbFormat {
  bool planar, reorder;     // [3][h][w] planes, else [h][w][3|4] words; BGR words / G, B, R planes
  int bytes, depth;         // per sample: 1 or 2; bits of a level: 8, 10, 12 or 16 (0: the format names none of them)
};
bool frame_rgb_format(int format, RgbFormat* f);
int frame_rgb_check(const char* what, const void* ptr, const dvsr_frame_desc* d, int Ht, int Wt, bool emit);
int frame_rgb_ingest_launch(const void* src, const dvsr_frame_desc& sd, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st);
int frame_rgb_emit_launch(const float* src, int Hs, int Ws, void* dst, const dvsr_frame_desc& dd, float lo, float hi, hipStream_t st);

// task.hip: the table of dvsr_task_degrade (degrade.hip) and dvsr_task_gather -- null, n, format, pixel stride, and every row of
// the HOST copy: source, strides, fp32 alignment, flags (DVSR_TASK_TRANSPOSE only where `square`), kernel index (n_kernels = 0:
// not looked at).  Launches nothing.
int task_table_check(const char* what, const dvsr_task_frame* items, const dvsr_task_frame* items_dev, int n, int format,
                     int pixel_stride, int H, int W, int n_kernels, bool square);

// frame_yuv.hip: the same pair for a YCbCr 4:2:0, 4:2:2 or 4:4:4 frame of 8, 10 or 12 bits (planes at any address / pitch), on
// the one form that both public descriptors take inside.  yuv_frame_from checks the descriptor's own part -- null, format,
// depth -- and fills it; _check does the rest.
struct YuvFrame {
  void* plane[3];
  long long rs[3];          // row strides, bytes
  int h, w, matrix, range;
  bool semi;                // interleaved CbCr (NV12 / NV16, P010 / P012 / P210 / P212); otherwise planar
  int bytes, depth;         // per sample: 1 or 2; bits of a level: 8, 10 or 12
  int chroma;               // DVSR_YUV_CHROMA_420 / _422 / _444 (never semi-planar)
  int siting;               // YUV_SITE_*: where a chroma sample sits (4:4:4: left, unused)
};
// the chroma field of a descriptor's format names a pair: yuv_frame_from splits it into `chroma` and `siting`
enum : int { YUV_SITE_LEFT = 0, YUV_SITE_CENTER = 1, YUV_SITE_TOPLEFT = 2 };
int yuv_frame_from(const char* what, const dvsr_yuv_desc* d, YuvFrame* f);
int yuv_frame_from(const char* what, const dvsr_yuv16_desc* d, YuvFrame* f);
int frame_ingest_yuv_check(const char* what, const YuvFrame& f, const float* dst, int Hp, int Wp, int pad_mode);
int frame_ingest_yuv_launch(const YuvFrame& f, float* dst, int Hp, int Wp, int pad_mode, hipStream_t st);

// pad.hip: explicit padding / layout changes of the MFDN estimator and their adjoints
enum : int { PAD_REFLECT = 0, PAD_REFLECT_S2D = 1, PAD_REPL_T3 = 2 };
size_t pad_out_numel(int mode, size_t N, int C, int H, int W);
int pad_fwd(const float* x, float* y, int mode, int N, int C, int H, int W, int T, hipStream_t st);
int pad_bwd(const float* gy, float* gx, int mode, int N, int C, int H, int W, int T, int accumulate,
            hipStream_t st, const float* gmask = nullptr, int gmask_act = 0, int gmask_padded = 0);
int meansub_slices();  // scratch floats per plane
int meansub_fwd(const float* x, float* xm, float* mean, float* part, int B, int C, int T, int H, int W,
                hipStream_t st);
int addmean_fwd(const float* y, const float* mean, float* out, int B, int C, int T, size_t HW, hipStream_t st);
int addmean_bwd(const float* gout, float* gy, int B, int C, int T, size_t HW, hipStream_t st);
int w4_to_s2d(const float* w, float* w2, int Cout, int C, int inverse, hipStream_t st);

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// Sampling geometry of one (pixel, tap) of the deformable conv: 4 corner offsets and weights;
// an invalid corner contributes 0 (deform_conv_cuda_kernel.cu:479-490).
struct DcnTap {
  int o1, o2, o3, o4;    // element offsets inside a plane (0 when the corner is invalid)
  float w1, w2, w3, w4;  // hh*hw, hh*lw, lh*hw, lh*lw
  float lh, lw;
  bool v1, v2, v3, v4;
};

// false <=> the sample is outside the (-1,H)x(-1,W) gate (kernel.cu:617) and contributes nothing.
__device__ __forceinline__ bool make_tap(float h_im, float w_im, int H, int W, DcnTap& t) {
  if (!(h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W)) return false;
  const int h_lo = (int)floorf(h_im), w_lo = (int)floorf(w_im);
  const int h_hi = h_lo + 1, w_hi = w_lo + 1;
  t.lh = h_im - (float)h_lo;
  t.lw = w_im - (float)w_lo;
  const float hh = 1.f - t.lh, hw = 1.f - t.lw;
  t.v1 = h_lo >= 0 && w_lo >= 0;
  t.v2 = h_lo >= 0 && w_hi <= W - 1;
  t.v3 = h_hi <= H - 1 && w_lo >= 0;
  t.v4 = h_hi <= H - 1 && w_hi <= W - 1;
  t.o1 = t.v1 ? h_lo * W + w_lo : 0;
  t.o2 = t.v2 ? h_lo * W + w_hi : 0;
  t.o3 = t.v3 ? h_hi * W + w_lo : 0;
  t.o4 = t.v4 ? h_hi * W + w_hi : 0;
  t.w1 = hh * hw; t.w2 = hh * t.lw; t.w3 = t.lh * hw; t.w4 = t.lh * t.lw;
  return true;
}

}  // namespace dvsr
