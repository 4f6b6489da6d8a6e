/*
 * semseg_hip.h -- C ABI of libsemseg_hip.so, the gfx950 (MI355X / CDNA4) kernel
 * library underneath the HRNet-OCR-MScale hot path.
 *
 * The reference (NVIDIA/semantic-segmentation) has no FFI of its own: every
 * arithmetic op on the hot path is a PyTorch/cuDNN/apex call made from Python
 * (SURVEY.md section 2b, rows K1..K15).  Each entry point below replaces one of
 * those call sites; the reference file:line is cited per function.  The Python
 * binding is ctypes (semseg_amd/_lib.py): plain pointers, ints and a
 * hipStream_t passed as void*.  No torch types cross this boundary.
 *
 * Conventions
 *  - every function returns 0 on success, SSA_EINVAL(-1)/SSA_EUNSUPPORTED(-2)
 *    for bad arguments, or a positive hipError_t.
 *  - all pointers are DEVICE pointers borrowed for the duration of the call;
 *    nothing is allocated, freed, retained or synchronised inside the library
 *    (hipGraph-capture safe, callable from the autograd thread).
 *  - activations are NHWC.  "ld" arguments are the pixel stride in elements so
 *    a tensor may be a channel slice of a wider buffer (concat-free writes).
 *  - bf16 tensors are 16-bit words, 16-byte aligned, channel count % 8 == 0.
 */
#ifndef SEMSEG_HIP_H
#define SEMSEG_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSA_OK 0
#define SSA_EINVAL (-1)
#define SSA_EUNSUPPORTED (-2)

int ssa_version(void);
/* Storage format of the 16-bit activations this build was compiled for (csrc/common.h): 0 = bf16
 * (libsemseg_hip.so), 1 = fp16 (libsemseg_hip_f16.so, -DSSA_ELEM_F16; the reference's --fp16 / apex O1 format,
 * train.py:381).  Every `bf16` in the names and comments below reads "the build's 16-bit element".            */
int ssa_elem_type(void);
/* First 16 hex digits of sha256 over the kernel sources the library was built from (csrc/Makefile): the Python
 * loader recomputes it over the sources next to the binary and refuses a stale build.                          */
const char* ssa_source_sha(void);

/* ------------------------------------------------------- grouped launches --
 * The 2-4 resolution branches of a HighResolutionModule (network/hrnetv2.py:181-254)
 * times the scale passes of MscaleOCR (network/ocrnet.py:264-327) are independent
 * problems that the reference issues as separate cuDNN/ATen calls.  Between
 * ssa_group_begin() and ssa_group_end(stream) the group-aware entry points (convolutions,
 * BatchNorm passes, sums, bilinear resampling, weight gradients) queue their launch on
 * the calling thread instead of issuing it; ssa_group_end issues ONE launch per kernel
 * instantiation covering all queued problems (job table in the kernel arguments).
 * Contract: launches queued in one bracket are mutually independent.  Other entry
 * points launch immediately.  Brackets nest (the outermost end flushes);
 * ssa_group_abort drops a bracket after a host-side error.
 * ssa_launch_count: kernel launches issued by this library so far (reset != 0 clears). */
int ssa_group_begin(void);
int ssa_group_end(void* stream);
int ssa_group_abort(void);
long ssa_launch_count(int reset);

/* Per-launch timing for the roofline measurement (bench.py): between ssa_profile_begin and
 * ssa_profile_end every launch of a group-aware kernel (all convolution-class kernels,
 * BatchNorm, sums, resampling) is bracketed by HIP events on the stream it is launched on.
 * ssa_profile_note attaches algorithmic flops / HBM bytes to the NEXT job submitted by the
 * calling thread.  ssa_profile_end waits for the device and returns one aggregate record
 * per kernel instantiation (name as rocprofv3 prints the template arguments).            */
typedef struct ssa_profile_rec {
  char kernel[120];
  long launches, jobs;
  double total_us, flops, bytes;
} ssa_profile_rec;
int ssa_profile_begin(void);
int ssa_profile_note(double flops, double bytes);
int ssa_profile_end(ssa_profile_rec* out, int max_recs);

/* ------------------------------------------------------------------ conv --
 * Implicit-GEMM convolution on MFMA (v_mfma_f32_32x32x16_bf16), NHWC bf16 in,
 * fp32 accumulate, bf16 or fp32 out.  Replaces nn.Conv2d forward / dgrad /
 * wgrad at network/hrnetv2.py:31-34,42-45,76-77,270-275 (K1,K2),
 * network/ocrnet.py:54-58 (K3), network/utils.py:348-357 (K4), every 1x1 in
 * network/ocr_utils.py:68-93,142-147 (K5) and the dilated ASPP convs at
 * network/utils.py:192-198 (K6). */
typedef struct ssa_conv_desc {
  int B, H, W, Cin;   /* input  [B,H,W,Cin], Cin % 8 == 0                      */
  int ldx;            /* input pixel stride (elements)                         */
  int Ho, Wo, Cout;   /* output [B,Ho,Wo,Cout]                                 */
  int ldy;            /* output pixel stride (elements)                        */
  int KH, KW;         /* filter taps                                           */
  int stride, pad, dil;
  int transposed;     /* 0: iy = oy*stride - pad + kh*dil   (forward)
                         1: iy = (oy - pad + kh*dil)/stride when divisible
                            (data-gradient of a strided forward conv)          */
  int Kpad;           /* row length of the packed filter matrix (multiple of 32) */
  int out_f32;        /* 0: bf16 output, 1: fp32 output                        */
  int cfg;            /* tile configuration id, -1 = choose automatically       */
} ssa_conv_desc;

/* y[m, n] = bias[n] + sum_k A[m, k] * Wp[n, k];  m=(b,oy,ox), k=(kh,kw,ci). */
int ssa_conv2d_igemm(const ssa_conv_desc* d, const void* x, const void* w_packed,
                     const float* bias, void* y, void* stream);

/* Same, with the BatchNorm batch statistics of the bf16-rounded outputs accumulated in
 * the epilogue (stats: [ssa_bn_stat_replicas()][2][Cout] fp64, caller clears; bf16
 * output, forward form only) -- replaces the ssa_bn_stats pass after the conv.        */
int ssa_conv2d_igemm_stats(const ssa_conv_desc* d, const void* x, const void* w_packed,
                           const float* bias, void* y, double* stats, void* stream);

/* Halo-tile convolution for the small-channel 3x3 stride-1 "same" convs of the
 * HRNet branches (Cin in {48, 64, 96}): the input halo tile is staged in LDS
 * once, all taps are computed from it, the filter streams from L2 in fragment
 * order (ssa_pack_filter mode 2/3).  stats (optional): BatchNorm partial sums
 * [ssa_bn_stat_replicas()][2][Cout] fp64, ACCUMULATED (caller clears), of the
 * bf16-rounded outputs -- the conv epilogue replaces the ssa_bn_stats pass.
 * ssa_conv2d_tile_supported: 1 if this descriptor can run on this kernel.     */
int ssa_conv2d_tile_supported(const ssa_conv_desc* d);
int ssa_conv2d_tile(const ssa_conv_desc* d, const void* x, const void* w_frag,
                    const float* bias, void* y, double* stats, void* stream);
int ssa_bn_stat_replicas(void);
/* The same convolution as the DATA GRADIENT of a residual block's conv (flipped, transposed
 * filter: ssa_pack_filter mode 3), with a second tile `aux` ([B,H,W,>=Cout] bf16, pixel stride
 * ldaux), congruent with the output, folded into the epilogue:
 *   aux_mode 1: y = bf16(bf16(conv) + aux) -- the gradient of the identity branch
 *               (network/hrnetv2.py:58-64 `out += residual`) added where autograd would launch
 *               a separate add; stats must be NULL.
 *   aux_mode 2: aux is the input x of the BatchNorm+ReLU layer whose output this conv consumed
 *               (conv1 -> bn1 -> relu -> conv2, network/hrnetv2.py:44-56); besides y = dz the
 *               epilogue ACCUMULATES that layer's backward sums into stats
 *               [ssa_bn_stat_replicas()][2][Cout] fp64:  sum(m*dz), sum(m*dz*xhat),
 *               m = [coef[0][c]*x + coef[1][c] > 0], xhat = (x - coef[2][c]) * coef[3][c]
 *               (coef = the [4][Cout] table ssa_bn_apply_train wrote) -- replaces the
 *               ssa_bn_bwd_reduce pass over (x, dz) of that layer.
 * Same shape support as ssa_conv2d_tile.                                                  */
int ssa_conv2d_tile_aux(const ssa_conv_desc* d, const void* x, const void* w_frag,
                        const float* bias, void* y, double* stats, const void* aux, int ldaux,
                        const float* coef, int aux_mode, void* stream);

/* Persistent, software-pipelined form of ssa_conv2d_tile / ssa_conv2d_tile_aux for the trunk's 48/96/192/384-channel
 * 3x3 convs (csrc/conv_tile_p.hip): a workgroup walks a strip of tiles of one (problem, 32-channel n-block), the input
 * in chunks of 48 channels, the filter streamed as one continuous LDS-DMA pipeline through a ring of three buffers,
 * the next halo in flight during the MFMAs, a register-only epilogue (swapped MFMA operands + v_permlane32_swap) and
 * the BatchNorm statistics in registers over the strip; three workgroups per CU.  No bias (SSA_EUNSUPPORTED).
 * stats / aux / aux_mode / coef as ssa_conv2d_tile_aux (aux_mode 0: none).
 * aux_mode 3 / 4 (inference; stats NULL): the conv's BatchNorm in evaluation mode as the epilogue -- z = scale * y + shift
 * (+ aux, the residual tile, when given), 4: followed by the ReLU; coef = the layer's [4][Cout] table (rows 0, 1 = scale,
 * shift: ssa_bn_finalize / ssa_bn_finalize_eval_batched); y is rounded to 16 bits first, so z equals ssa_bn_apply on the
 * stored conv output bit for bit.  conv -> bn -> relu of network/hrnetv2.py:37-66 in eval() as one launch.
 * ssa_conv_tile_strip(units): work (in units of one 128-pixel tile x one 48-channel chunk x one n-block = 27 MFMAs
 * per wave) a workgroup of the calling thread's NEXT launches should carry -- the caller of a grouped level knows the
 * level's total; 0 = derive from each problem alone.                                                              */
int ssa_conv2d_tile_p_supported(const ssa_conv_desc* d);
int ssa_conv_tile_strip(int units);
int ssa_conv2d_tile_p(const ssa_conv_desc* d, const void* x, const void* w_frag, const float* bias, void* y,
                      double* stats, const void* aux, int ldaux, const float* coef, int aux_mode, void* stream);

/* Large-channel 3x3 / 1x1 stride-1 "same" convs of the OCR and attention heads
 * (Cin >= 192, Cin % 48 == 0 or % 64 == 0).  1x1: halo-chunk implicit GEMM,
 * 256-pixel x 128-channel workgroup tiles, the input tile of each 48/64 channel
 * chunk staged in LDS, the filter (fragment order, ssa_pack_filter mode 2/3)
 * streamed by global_load_lds; bf16 or fp32 output.  3x3: forwarded to
 * ssa_conv2d_halo_reg, so only the problems it supports are supported here.
 * stats as for ssa_conv2d_tile (bf16 output only).                             */
int ssa_conv2d_halo_supported(const ssa_conv_desc* d);
int ssa_conv2d_halo(const ssa_conv_desc* d, const void* x, const void* w_frag,
                    const float* bias, void* y, double* stats, void* stream);

/* Wide-tile GEMM for the large 1x1 stride-1 convs of the OCR / attention heads and their data gradients (aux_head
 * 720->720, SpatialOCR 1024->512, f_up 256->512; network/ocrnet.py:61-76, network/ocr_utils.py:68-93,142-156):
 * 256 pixels x 256 output channels per workgroup, 128 x 64 per wave (4 x 2 MFMA 32x32x16 tiles), both operands by
 * global_load_lds in 32-channel stages through a ring of four LDS buffers (csrc/conv_gemm_wide.hip).  Same operands
 * as ssa_conv2d_halo (w_frag: ssa_pack_filter mode 2 / 3 with cin_pad = d->Cin, a multiple of 16); 16-bit output
 * only; stats as for ssa_conv2d_tile.  ssa_conv2d_halo forwards the problems for which
 * ssa_conv2d_gemm_wide_supported() returns 1 (1x1, more than 256 output channels, >= 16384 pixels; SSA_GEMM_WIDE=0
 * keeps them on the 256 x 128 kernel); the entry point itself takes any 1x1 stride-1 problem of >= 256 pixels.   */
int ssa_conv2d_gemm_wide_supported(const ssa_conv_desc* d);
int ssa_conv2d_gemm_wide(const ssa_conv_desc* d, const void* x, const void* w_frag, const float* bias,
                         void* y, double* stats, void* stream);

/* Register-fed kernel for the 3x3 stride-1 "same" convs of the OCR / attention heads and their data gradients
 * (conv3x3_ocr 720->512, attn 512->256 / 256->256; network/ocrnet.py:54-58, network/utils.py:348-357): 128 pixels x
 * 256 channels per 4-wave workgroup, 128 x 64 per wave (4 x 2 MFMA 32x32x16 tiles); the filter fragments go straight
 * from global memory into the MFMA operand registers through a ring six k-steps deep (they never touch LDS), the input
 * halo tile by LDS DMA, double buffered per 48 / 64-channel chunk: one workgroup barrier per chunk
 * (csrc/conv_halo_reg.hip).  Same operands as ssa_conv2d_halo; 16-bit output only; stats as for ssa_conv2d_tile.
 * ssa_conv2d_halo forwards every 3x3 problem here.                                                                */
int ssa_conv2d_halo_reg_supported(const ssa_conv_desc* d);
int ssa_conv2d_halo_reg(const ssa_conv_desc* d, const void* x, const void* w_frag, const float* bias,
                        void* y, double* stats, void* stream);

/* 5x5 stride-1 pad-2 convs of the Deeper (Panoptic-DeepLab style) decoders and their data gradients (conv_up2 320->256
 * at stride 4, conv_up3 288->256 at stride 2: cuDNN behind ConvBnRelu(.., kernel_size=5, padding=2) at
 * network/deeper.py:53-54 and network/mscale.py:382-383).  The kernel of ssa_conv2d_halo_reg with 25 taps: 128 pixels x
 * 256 channels per 4-wave workgroup, filter fragments from global memory straight into the MFMA registers, the 8 x 36
 * pixel halo tile of each 48 / 64-channel chunk by LDS DMA, double buffered: one workgroup barrier per chunk
 * (csrc/conv_halo5.hip).  Same operands as ssa_conv2d_halo_reg (w_frag: ssa_pack_filter mode 2 / 3, k = (kh, kw, ci),
 * Kpad = 25 * Cin); Cin % 48 == 0 or % 64 == 0; 16-bit output only; stats as for ssa_conv2d_tile.
 * ssa_conv2d_halo5_supported() adds the size policy (W >= 32 and >= 16384 pixels: smaller problems stay on
 * ssa_conv2d_igemm); the entry point itself takes any size.                                                         */
int ssa_conv2d_halo5_supported(const ssa_conv_desc* d);
int ssa_conv2d_halo5(const ssa_conv_desc* d, const void* x, const void* w_frag, const float* bias,
                     void* y, double* stats, void* stream);

/* Tile configuration ssa_conv2d_igemm would use for this problem
 * (0: 128x128, 1: 256x64, 2: 128x96, 3: 256x32, 4: 64x64, 5: 128x64 tiles). */
int ssa_conv2d_igemm_tile(const ssa_conv_desc* d);
/* ssa_conv2d_igemm with the conv's BatchNorm in evaluation mode as the epilogue (inference): z = scale * y + shift
 * (+ residual [B,Ho,Wo,Cout], pixel stride ldres) and, relu != 0, the ReLU; coef = the layer's [4][Cout] table (rows 0, 1);
 * y = the conv output (+ bias) rounded to 16 bits first, so z equals ssa_bn_apply on the stored output bit for bit.
 * 16-bit output, not transposed.  conv -> bn (-> relu) of the stem, layer1 and the fuse layers
 * (network/hrnetv2.py:278-300, 192-222) in eval() as one launch.                                                  */
int ssa_conv2d_igemm_affine(const ssa_conv_desc* d, const void* x, const void* w_packed, const float* bias, void* y,
                            const float* coef, const void* residual, int ldres, int relu, void* stream);


/* Data gradient of a 3x3, stride-2, pad-1 convolution (the fuse / transition / stem
 * down-convs of network/hrnetv2.py:218-250, 357-371; cuDNN's backward-data behind
 * nn.Conv2d) decomposed by OUTPUT PARITY: the pixels (2m+py, 2n+px) of dx depend on
 * (1+py)*(1+px) of the 9 taps only, so the four classes are four dense stride-1
 * correlations of dy with 1, 2, 2 and 4 taps -- no multiplications by the zeros of the
 * zero-inserted form (ssa_conv2d_igemm with transposed = 1 does 4x the MFMA work).
 * dy: [B,Ho,Wo,cout_pad] bf16 (row stride lddy), dx: [B,H,W,Cin] bf16 (lddx), every pixel
 * written.  w_cls[c], kpad_cls[c]: operand of class c = 2*py+px packed by
 * ssa_pack_filter(mode 4+c) -- [Cin][Kpad], k = (jy, jx, co).  Inside a group bracket the
 * four problems share one launch.                                                        */
int ssa_conv2d_dgrad_s2(int B, int H, int W, int Cin, int lddx, int Ho, int Wo, int cout_pad,
                        int lddy, const void* dy, const void* const* w_cls, const int* kpad_cls,
                        void* dx, void* stream);

/* Filter packing: OIHW fp32 parameter -> bf16 [rows][Kpad] GEMM operand.
 * mode 0 (forward): rows = Cout, k = (kh,kw,ci) with ci < cin_pad.
 * mode 1 (dgrad)  : rows = Cin,  k = (kh',kw',co) with co < cout_pad, taps
 *                   flipped (kh' = KH-1-kh) -- the transposed filter.
 * mode 2 / 3      : the same two operands in MFMA-fragment order for
 *                   ssa_conv2d_tile: [n-block][k-step][lane][8], rows padded to
 *                   a multiple of 32, Kpad = KH*KW*c_pad (a multiple of 16).
 * mode 4 + 2*py + px (3x3 only): data-gradient operand of parity class (py, px) of a
 *                   stride-2 conv (ssa_conv2d_dgrad_s2): rows = Cin,
 *                   k = (jy, jx, co), jy <= py, jx <= px, co < cout_pad; tap j of
 *                   class 0 is forward tap 1, of class 1 forward tap 2 - 2j.       */
int ssa_pack_filter(const float* w_oihw, void* w_packed, int Cout, int Cin,
                    int KH, int KW, int cin_pad, int cout_pad, int Kpad,
                    int mode, void* stream);

/* Weight gradient, split over the pixel axis.  partial is
 * [nsplit][cout_pad][KH*KW*Cin] fp32; ssa_conv2d_wgrad_reduce sums the splits
 * and writes dW in the parameter's OIHW fp32 layout (cin_real <= d->Cin);
 * accumulate != 0: ADDS to dW instead (dW = the layer's slice of the step's gradient
 * arena, cleared once per step; the passes of a multi-scale step write their splits
 * behind one another in `partial` and ONE reduce sums them all).
 * The weight-gradient kernels and the reduce are group-aware: the host defers a
 * module's weight gradients and issues them inside one ssa_group bracket.
 * d->cfg > 0 in the *_plan calls: bound a workgroup's pixel strip to cfg 128-pixel
 * stages instead of splitting for parallelism (grouped launches get their
 * parallelism from the number of layers).                                     */
int ssa_conv2d_wgrad_plan(const ssa_conv_desc* d, int cout_pad, int* nsplit,
                          size_t* ws_bytes);
int ssa_conv2d_wgrad(const ssa_conv_desc* d, const void* x, const void* dy,
                     int lddy, int cout_pad, int nsplit, float* partial,
                     void* stream);
int ssa_conv2d_wgrad_reduce(const float* partial, int nsplit, int cout_pad,
                            int Cout, int Cin_pad, int Cin, int KH, int KW,
                            float* dw_oihw, int accumulate, void* stream);

/* All filters of a network repacked in ONE launch (the parameters change every
 * optimizer step; 1,276 separate pack launches cost more than the packing).
 * jobs_dev: device array of ssa_pack_job; same semantics as ssa_pack_filter.  */
typedef struct ssa_pack_job {
  const float* w_oihw;
  void* w_packed;
  long elem_begin;   /* ssa_pack_filters_tiled: 1 + index of the next job packed from the same OIHW tensor (its tiles
                      * are then NOT listed: the owner's workgroups write every chained form from one read); 0: none.
                      * ssa_pack_filters_batched ignores it                                                   */
  int Cout, Cin, KH, KW, cin_pad, cout_pad, Kpad, mode, rows;
  int layout;        /* reserved, 0: mode 2 / 3 write the one fragment order of conv_tile(_p).hip / conv_halo_gemm.hip */
} ssa_pack_job;
int ssa_pack_filters_batched(const void* jobs_dev, int njobs, int blocks_per_job,
                             void* stream);
/* The same repack balanced by TILE: tiles_dev = device array of int4 {job index, first output
 * channel (multiple of 32), first input channel (multiple of ct), ct} covering every job's
 * [Cout] x [Cin] plane with 32 x ct tiles, ct = ssa_pack_tile_channels(KH, KW) (0: filter
 * too large for this path -> use ssa_pack_filters_batched).  Writes the data elements only:
 * the destinations' zero padding must be in place (cleared buffers packed once by
 * ssa_pack_filter).  max_ct_taps = the largest ct * KH * KW over the tiles (sizes the LDS
 * tile).  One coalesced read of each OIHW tile serves either operand form.                 */
int ssa_pack_tile_channels(int KH, int KW);
int ssa_pack_filters_tiled(const void* jobs_dev, const void* tiles_dev, int ntiles,
                           int max_ct_taps, void* stream);

/* Halo-staged weight gradient for the 3x3 stride-1 trunk convs with
 * Cin == cout_pad in {48, 64, 96, 192, 384}: persistent workgroups keep their
 * block of dW in MFMA accumulators while they walk 128-pixel tiles whose x halo
 * image and dy tile are staged in LDS once (transposing ds_read_b64_tr_b16
 * fragment reads).  Same partial layout as ssa_conv2d_wgrad
 * ([nsplit][cout_pad][9*Cin] fp32) -> finish with ssa_conv2d_wgrad_reduce.
 * _plan returns SSA_EUNSUPPORTED for shapes this kernel does not take.          */
int ssa_conv2d_wgrad_tile_plan(const ssa_conv_desc* d, int cout_pad, int* nsplit,
                               size_t* ws_bytes);
int ssa_conv2d_wgrad_tile(const ssa_conv_desc* d, const void* x, const void* dy,
                          int lddy, int cout_pad, int nsplit, float* partial,
                          void* stream);
/* Launch geometry of ssa_conv2d_wgrad_tile for a Cin = cout_pad layer, for the host's strip fitting
 * (hip_backend._fit_tile_strips): parts = workgroups per strip of 128-pixel tiles, slots = workgroups of that
 * instantiation resident on the chip at once, kind = which instantiation (launches of one kind share a grouped launch:
 * 0 = the 8-wave all-taps form of the 96-channel blocks, csrc/conv_wgrad_tile.hip ConvWgradTileA). */
int ssa_conv2d_wgrad_tile_geometry(int Cin, int cout_pad, int* parts, int* slots, int* kind);
/* Weight gradient of the large-channel 3x3 / 1x1 stride-1 head convs (Cin >= 128,
 * >= 16 K pixels): 8-wave workgroups persistent over 128-pixel tiles hold a
 * 128(co) x 128(ci) x 3(kw) [3x3] or 128 x 256 [1x1] block of dW in MFMA
 * accumulators; LDS images pixel-major, transposing fragment reads.  Partial
 * layout as ssa_conv2d_wgrad -> finish with ssa_conv2d_wgrad_reduce.            */
int ssa_conv2d_wgrad_head_plan(const ssa_conv_desc* d, int cout_pad, int* nsplit,
                               size_t* ws_bytes);
int ssa_conv2d_wgrad_head(const ssa_conv_desc* d, const void* x, const void* dy,
                          int lddy, int cout_pad, int nsplit, float* partial,
                          void* stream);

/* Column sum over pixels: out[c] = sum_p x[p, c]  (bias gradient). x bf16. */
int ssa_colsum_bf16(const void* x, long P, int C, int ld, float* out,
                    double* scratch2c, void* stream);

/* fp32 [P,C] -> bf16 [P,Cpad] zero padded (gradient of the fp32 heads). */
int ssa_pad_cast_f32_bf16(const float* x, long P, int C, int ldx, void* y,
                          int Cpad, void* stream);

/* --------------------------------------------------------------- batchnorm --
 * Replaces cfg.MODEL.BNFUNC (nn.BatchNorm2d / apex SyncBatchNorm) selected at
 * config.py:216-225 and instantiated by network/mynn.py:18-24 (K7, C3).      */
/* sums[0:C] += sum_p x, sums[C:2C] += sum_p x^2 (fp64).  zero_sums=1 clears sums
 * first (one memset per call); callers that carve sums out of an arena they
 * clear once per step pass 0.                                                  */
int ssa_bn_stats(const void* x, long P, int C, int ld, double* sums, int zero_sums,
                 void* stream);
/* Training-mode normalisation with the finalize step fused in (one launch):
 * z = post*act(bn(x) + residual) with batch statistics from `sums`/`count`
 * (possibly all-reduced: SyncBN).  sums is [nrep][2][C]: nrep = 1 after
 * ssa_bn_stats, ssa_bn_stat_replicas() after a conv epilogue
 * (ssa_conv2d_tile) -- the replicas are summed here.  Writes coef = [scale|shift|mean|invstd] (4*C
 * fp32) for the backward pass.  Running statistics: either updated here
 * (running_mean/var + *num_batches_tracked given; momentum, unbiased variance)
 * or deferred: pass_stats (2*C+1 fp32: mean, biased var, count) is filled and
 * ssa_bn_update_running_batched applies every layer's passes in order later
 * -- required when passes over the same layer run on concurrent streams.      */
int ssa_bn_apply_train(const void* x, int ldx, const void* residual, int ldr, void* z,
                       int ldz, long P, int C, const double* sums, int nrep, double count,
                       const float* gamma, const float* beta, float* running_mean,
                       float* running_var, long* num_batches_tracked, float momentum,
                       float eps, float* coef, float* pass_stats, int relu,
                       const float* post, long pix_per_img, void* sign_mask, void* stream);
/* sign_mask (optional, [P][C/8] bytes): bit j of byte (p, g) = z[p][8g + j] > 0 as stored.  Handed to the two
 * backward passes below in place of z: behind a residual add the ReLU mask cannot be recomputed from x alone
 * (mask_scale / mask_shift), and reading 1 byte instead of 16 per piece takes 28 MB off the 118 MB a trunk
 * level's bn2 backward moves.                                                                               */
typedef struct ssa_bn_update_job {
  float* running_mean;
  float* running_var;
  long* num_batches_tracked;
  const float* pass_stats[8];
  int C, npass;
  float momentum;
  int pad_;
} ssa_bn_update_job;
/* jobs_dev: device array of ssa_bn_update_job; one launch for all layers.     */
int ssa_bn_update_running_batched(const void* jobs_dev, int njobs, int max_channels,
                                  void* stream);
/* Evaluation-mode coefficients of many layers in one launch (use_running = 1 of ssa_bn_finalize, the same arithmetic):
 * coef = [4][C] scale, shift, mean, invstd.  nn.BatchNorm2d.eval() of the reference (network/mynn.py:18-24) computes them
 * inside every cuDNN call; here they were one launch per layer and scale pass.  jobs_dev: device array.            */
typedef struct ssa_bn_eval_job {
  const float* gamma;          /* NULL: 1 */
  const float* beta;           /* NULL: 0 */
  const float* running_mean;
  const float* running_var;
  float* coef;
  int C;
  float eps;
} ssa_bn_eval_job;
int ssa_bn_finalize_eval_batched(const void* jobs_dev, int njobs, int max_channels, void* stream);
/* From (possibly all-reduced) sums and total count: scale/shift for the apply
 * pass, mean/invstd for backward, running-stat update (momentum, unbiased var).
 * use_running=1 (eval): scale/shift from running stats, sums ignored.          */
int ssa_bn_finalize(const double* sums, double count, int C, const float* gamma,
                    const float* beta, float* running_mean, float* running_var,
                    float momentum, float eps, int use_running, float* scale,
                    float* shift, float* mean, float* invstd, void* stream);
/* z = post[b,c] * act(scale[c]*x + shift[c] + residual)                       */
int ssa_bn_apply(const void* x, int ldx, const void* residual, int ldr, void* z,
                 int ldz, long P, int C, const float* scale, const float* shift,
                 int relu, const float* post, long pix_per_img, void* stream);
/* mask_scale/mask_shift (both backward passes, optional): the ReLU mask is recomputed
 * as scale[c]*x + shift[c] > 0 (the forward's own coefficients) instead of read from
 * z -- z may then be NULL: one tensor less to read, and to keep, per BN+ReLU layer.
 * backward pass 1: sum g and sum g*xhat, g = dz*post*(z>0), accumulated into
 * sums[nrep][2][C] (workgroup b adds into replica b % nrep: fewer same-address
 * fp64 atomics); ssa_bn_bwd_apply sums the replicas.                           */
int ssa_bn_bwd_reduce(const void* x, int ldx, const void* dz, int lddz,
                      const void* z, int ldz, long P, int C, const float* mean,
                      const float* invstd, int relu, const float* post,
                      long pix_per_img, double* sums, int nrep, int zero_sums,
                      const float* mask_scale, const float* mask_shift, const void* sign_mask, void* stream);
/* backward pass 2: dx = gamma*invstd*(g - sum_g/N - xhat*sum_gxhat/N);
 * dres (optional) = g.  sums may have been all-reduced; count is global.
 * dgamma/dbeta (optional): = param_grad_scale * sums[C:2C] / sums[0:C]
 * (1/world under SyncBN, so that DDP's mean over ranks is unchanged);
 * accumulate_param_grads: ADD them (fp32 atomics) into buffers the caller cleared --
 * the gradient arena of the step, shared by every pass over the layer.        */
int ssa_bn_bwd_apply(const void* x, int ldx, const void* dz, int lddz,
                     const void* z, int ldz, void* dx, int lddx, void* dres,
                     int lddres, long P, int C, const float* gamma,
                     const float* mean, const float* invstd, const double* sums,
                     int nrep, double count, int relu, const float* post,
                     long pix_per_img, float* dgamma, float* dbeta,
                     float param_grad_scale, const float* mask_scale,
                     const float* mask_shift, int accumulate_param_grads, const void* sign_mask, void* stream);
/* ------------------------------------------------- pre-activation blocks ----
 * IdentityResidualBlock.forward (network/wider_resnet.py:172-185): the block input is a residual SUM, and it feeds
 * both bn1 and the shortcut (`shortcut = x.clone(); bn1 = self.bn1(x); ...; out.add_(shortcut)`), so the batch
 * statistics cannot ride on a conv epilogue and the input's gradient is bn1's dx plus the shortcut's.
 * forward: s[p,c] = round16(float(a) + float(b)) (16-byte pieces; bit for bit ssa_sum_act's), and
 * sums[0:C] += sum_p s, sums[C:2C] += sum_p s^2 over the values AS STORED: [1][2][C] fp64, what
 * ssa_bn_apply_train(..., nrep = 1) and the SyncBN exchange take.  One pass (read 2, write 1) for the sum pass and
 * the statistics pass (read 2 write 1, read 1).  a, b, s: 16-byte aligned, leading dimensions % 8 and >= C
 * (channel slices work); C % 8, C <= 2048.  zero_sums as in ssa_bn_stats.                                  */
int ssa_add_bn_stats(const void* a, int lda, const void* b, int ldb, void* s, int lds, long P,
                     int C, double* sums, int zero_sums, void* stream);
/* backward: ssa_bn_bwd_apply with dx = round16((A g + (Bx x + D)) + float(dadd)) -- the shortcut's gradient is a
 * fourth load stream of the pass and the sum is rounded once, instead of an add pass (read 2, write 1) behind it.
 * Built for the form that recomputes the ReLU mask from x (relu with mask_scale / mask_shift: the pre-activation
 * ReLU sits directly behind its BatchNorm); every other form returns SSA_EUNSUPPORTED.                    */
int ssa_bn_bwd_apply_add(const void* x, int ldx, const void* dz, int lddz,
                         const void* z, int ldz, void* dx, int lddx, void* dres,
                         int lddres, long P, int C, const float* gamma,
                         const float* mean, const float* invstd, const double* sums,
                         int nrep, double count, int relu, const float* post,
                         long pix_per_img, float* dgamma, float* dbeta,
                         float param_grad_scale, const float* mask_scale,
                         const float* mask_shift, int accumulate_param_grads, const void* sign_mask,
                         const void* dadd, int lddadd, void* stream);
/* dgamma[c] = sums[C+c], dbeta[c] = sums[c] (fp64 -> fp32)                     */
int ssa_bn_param_grads(const double* sums, int C, float* dgamma, float* dbeta,
                       void* stream);

/* ------------------------------------------------- SyncBN exchange, peer to peer ----
 * One-shot all-reduce (SUM, fp64, in place) of the SyncBN partial sums over peer-mapped device memory -- what
 * apex.parallel.SyncBatchNorm's all-reduce is in the reference (config.py:216-222, network/__init__.py:37-39) and
 * ncclAllReduce is on this path by default.  Every rank writes its n values into its slot of every peer's exchange
 * buffer, publishes a sequence number (system-scope release), waits for all peers' numbers in its own buffer and sums
 * the slots in rank order: one single-workgroup kernel on `stream`, capturable (the sequence number lives in *seq_dev and
 * is advanced by the kernel).  peers_dev: device array of `world` base addresses -- every rank's buffer as mapped into
 * THIS process (hipIpcOpenMemHandle; the rank's own allocation at [rank]); each buffer *bytes of ssa_p2p_buffer_bytes(world,
 * slot_doubles, &bytes) of zeroed fine-grained device memory.  n <= slot_doubles, else SSA_EUNSUPPORTED (the caller keeps
 * the collective library for those).  ssa_p2p_timeouts: ranks that gave up waiting (~2 s) -- 0 unless a peer died.
 * Host side: semseg_amd/p2p.py (opt-in, SSA_SYNCBN_P2P=1).                                                        */
int ssa_p2p_buffer_bytes(int world, long slot_doubles, size_t* bytes);
int ssa_p2p_allreduce_f64(double* data, long n, void* const* peers_dev, int rank, int world,
                          unsigned long long* seq_dev, long slot_doubles, void* stream);
int ssa_p2p_timeouts(unsigned* out);
/* Exchange buffers without hipIpc: *ptr = `bytes` (rounded up to the allocation granularity -> *mapped_bytes) of zeroed
 * uncached device memory on the current device, created through the virtual-memory API and exported as the POSIX file
 * descriptor *fd (the caller hands it to the peers over a unix socket, SCM_RIGHTS, and closes it).  A peer maps the
 * allocation with ssa_p2p_vmm_import(fd, mapped_bytes, &ptr) on ITS current device.  Needs no ptrace rights, which
 * hipIpcOpenMemHandle in dmabuf mode (pidfd_getfd) does.  SSA_EUNSUPPORTED when the runtime refuses every variant.   */
int ssa_p2p_vmm_alloc(size_t bytes, void** ptr, int* fd, size_t* mapped_bytes);
int ssa_p2p_vmm_import(int fd, size_t mapped_bytes, void** ptr);
int ssa_p2p_vmm_unmap(void* ptr, size_t mapped_bytes);

/* ----------------------------------------------------------- elementwise ---- */
/* z = relu?(a + b + c + d); b,c,d optional.  HRNet fuse sum,
 * network/hrnetv2.py:236-252 (K12). All bf16, dense [n] with n % 8 == 0.      */
int ssa_sum_act(const void* a, const void* b, const void* c, const void* d,
                void* z, long n, int relu, void* stream);
/* g = dz * (z > 0) */
int ssa_relu_bwd(const void* dz, const void* z, void* g, long n, void* stream);
/* NCHW fp32 image -> NHWC bf16 with channels zero-padded to cpad.
 * (train.py:487 hands the module an NCHW fp32 batch.)                         */
int ssa_nchw_f32_to_nhwc_bf16(const float* x, void* y, int B, int C, int H, int W,
                              int cpad, void* stream);

/* ResizeX(images, s) (network/mynn.py:101-114, called at network/ocrnet.py:276)
 * fused with the layout change: NCHW fp32 [B,C,Hi,Wi] -> NHWC bf16
 * [B,Ho,Wo,cpad]; Ho==Hi && Wo==Wi is an exact copy.                          */
int ssa_image_resize_to_nhwc_bf16(const float* x, int B, int C, int Hi, int Wi,
                                  void* y, int Ho, int Wo, int cpad, void* stream);
/* The same under either index rule of ResizeX (network/mynn.py:15 reads cfg.MODEL.ALIGN_CORNERS, the reference's
 * --align_corners): align_corners 0 is the entry point above, 1 is ATen's align_corners=True rule (scale =
 * (in - 1) / (out - 1), s = scale * o); any other value is SSA_EINVAL.            */
int ssa_image_resize_to_nhwc(const float* x, int B, int C, int Hi, int Wi,
                             void* y, int Ho, int Wo, int cpad, int align_corners, void* stream);

/* -------------------------------------------------------------- bilinear ----
 * F.interpolate(mode='bilinear', align_corners=False): network/mynn.py:42-114,
 * network/hrnetv2.py:246-249,440-445 (K8; align_corners=True: the ssa_resize_* entry points below).  in_dtype/out_dtype: 0 bf16, 1 f32.
 * Backward is a deterministic gather (no atomics).                             */
int ssa_bilinear_fwd(const void* x, int in_dtype, int B, int Hi, int Wi, int C,
                     int ldx, void* y, int out_dtype, int Ho, int Wo, int ldy,
                     void* stream);
int ssa_bilinear_bwd(const void* dy, int dy_dtype, int B, int Ho, int Wo, int C,
                     int lddy, void* dx, int dx_dtype, int Hi, int Wi, int lddx,
                     void* stream);
/* The same backward for an UPSAMPLING resize (Ho >= 2 Hi), separable (bilinear weights factor): pass X sums over the
 * output columns into tmp ([B, Ho, Wi, C] fp32, dense, 16-byte aligned), pass Y over the output rows -- window_x +
 * window_y taps per element instead of their product, dy read once.  Two dependent launches: never both in one
 * ssa_group bracket.  network/mynn.py:42-114 (Upsample / scale_as), network/hrnetv2.py:246-249,440-445.          */
int ssa_bilinear_bwd_x(const void* dy, int dy_dtype, int B, int Ho, int Wo, int C, int lddy, float* tmp, int Wi,
                       void* stream);
int ssa_bilinear_bwd_y(const float* tmp, int B, int Ho, int Wi, int C, void* dx, int dx_dtype, int Hi, int lddx,
                       void* stream);
/* The four entry points above under either index rule: F.interpolate(mode='bilinear', align_corners=
 * cfg.MODEL.ALIGN_CORNERS) -- the reference's --align_corners, read by network/mynn.py:15 (Upsample, Upsample2, scale_as,
 * ResizeX, DownX), network/hrnetv2.py:27, network/ocr_utils.py:117 and utils/trnval_utils.py:54.  align_corners 0: the
 * entry points above, bit for bit (they are calls of these with 0).  align_corners 1: ATen's rule, every step one fp32
 * operation: scale = out > 1 ? (in - 1) / (out - 1) : 0, s = scale * o, i0 = min((int)s, in - 1), i1 = i0 + (i0 < in - 1),
 * l1 = s - i0, l0 = 1 - l1.  scale == 0 (out == 1 or in == 1): every output reads input 0, whose gradient is the sum
 * of all output gradients.  An input pixel receives from up to ceil(2 / scale) outputs per axis (9 at 64 -> 256, 17 at
 * 128 -> 1024).  Same dtype routing, same refusals; align_corners outside {0, 1} is SSA_EINVAL.                     */
int ssa_resize_bilinear_fwd(const void* x, int in_dtype, int B, int Hi, int Wi, int C,
                            int ldx, void* y, int out_dtype, int Ho, int Wo, int ldy,
                            int align_corners, void* stream);
int ssa_resize_bilinear_bwd(const void* dy, int dy_dtype, int B, int Ho, int Wo, int C,
                            int lddy, void* dx, int dx_dtype, int Hi, int Wi, int lddx,
                            int align_corners, void* stream);
/* The separable pair (network/mynn.py:42-114, network/hrnetv2.py:246-249,440-445): pass X and pass Y of one resize take
 * the same align_corners.  Two dependent launches: never both in one ssa_group bracket.                              */
int ssa_resize_bilinear_bwd_x(const void* dy, int dy_dtype, int B, int Ho, int Wo, int C, int lddy, float* tmp, int Wi,
                              int align_corners, void* stream);
int ssa_resize_bilinear_bwd_y(const float* tmp, int B, int Ho, int Wi, int C, void* dx, int dx_dtype, int Hi, int lddx,
                              int align_corners, void* stream);

/* ----------------------------------------------------------------- pooling ----
 * DeepLabV3+/ResNet-50 (BASELINE configs[0]): nn.MaxPool2d(3, 2, 1) of the ResNet
 * stem (network/Resnet.py:147) and nn.AdaptiveAvgPool2d(1) of the ASPP image
 * branch (network/utils.py:201).  NHWC bf16, C % 8 == 0.  idx: winning tap per
 * output element (uint8, PyTorch's first-maximum rule), consumed by the backward. */
int ssa_maxpool3x3s2_fwd(const void* x, int ldx, int B, int H, int W, int C, void* y,
                         unsigned char* idx, int Ho, int Wo, void* stream);
int ssa_maxpool3x3s2_bwd(const void* dy, const unsigned char* idx, int B, int Ho, int Wo,
                         int C, void* dx, int H, int W, void* stream);
/* nn.MaxPool2d(3, stride=2, ceil_mode=True) without padding, the stem pool of the SE-ResNeXt trunks
 * (network/SEresnext.py:271-272): window rows 2 oy .. 2 oy + 2 and columns 2 ox .. 2 ox + 2 clipped to the image (a tap
 * past the edge never wins), Ho = H / 2, Wo = W / 2, H, W >= 2.  First-maximum / NaN rule and byte index map (tap =
 * kh * 3 + kw) of the padding-1 pool above.  16-byte aligned x, y, dy, dx (y, dy, dx dense), ldx % 8 == 0, >= C;
 * anything else returns -1 before the device is touched.                                                        */
int ssa_maxpool3x3s2c_fwd(const void* x, int ldx, int B, int H, int W, int C, void* y, unsigned char* idx, int Ho,
                          int Wo, void* stream);
int ssa_maxpool3x3s2c_bwd(const void* dy, const unsigned char* idx, int B, int Ho, int Wo, int C, void* dx, int H, int W,
                          void* stream);
/* out[b,c] = mean_p x[b,p,c];  dx[b,p,c] = dout[b,c] / HW                        */
int ssa_global_avg_pool_fwd(const void* x, int ldx, int B, long HW, int C, void* out,
                            void* stream);
int ssa_global_avg_pool_bwd(const void* dout, int B, long HW, int C, void* dx,
                            void* stream);

/* --------------------------------------------------------- grouped 3x3 conv ----
 * nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups = G, bias = False) with 1 < G < C: conv2 of every
 * SE-ResNeXt bottleneck (network/SEresnext.py:183-185; the stride-8 surgery of network/utils.py:71-81 sets dilation and
 * padding).  NHWC 16-bit, C % 8 == 0, Cg = C / G in {4, 8, 16, 32} (anything else: -2), pixel strides % 8 and >= C,
 * 16-byte aligned x, y, dy, dx (ssa_dwconv_desc's rules); w = the parameter's own [C][Cg][3][3] fp32 storage.  The
 * filter operand of the MFMA is 16-bit: the kernels round the fp32 parameter to the storage type (round to nearest
 * even), which is part of the contract.  A bad descriptor returns -1 before the device is touched.               */
typedef struct ssa_gconv_desc {
  int B, H, W, C, G, ldx;  /* x [B,H,W,C], G groups */
  int Ho, Wo, ldy;         /* y [B,Ho,Wo,C], Ho = (H-1)/stride + 1 */
  int stride, dil;         /* stride 1 with dil >= 1, or stride 2 with dil 1; padding = dil */
} ssa_gconv_desc;
/* y = round16(sum over the group's Cg input channels and the 9 taps of round16(w) x).  stats (training; replaces the
 * ssa_bn_stats pass of bn2): sum y and sum y^2 of the values AS STORED are added into [ssa_bn_stat_replicas()][2][C]
 * fp64 (caller clears) -- ssa_dwconv3x3's contract.                                                              */
int ssa_gconv3x3(const ssa_gconv_desc* d, const void* x, const float* w, void* y, double* stats, void* stream);
/* Backward of the same conv (cuDNN's backward-data and backward-filter behind the grouped nn.Conv2d): dx (nullable)
 * [B,H,W,C] 16-bit, every pixel written; dw (nullable) [C][Cg][3][3] fp32, added to when accumulate != 0, summed in a
 * fixed order.  ws: ssa_gconv3x3_bwd_plan's bytes (the workgroups' fp32 partial tiles of dw; needed with dw).  x is
 * needed with dw, w with dx.  Asking for neither returns -1.                                                    */
int ssa_gconv3x3_bwd_plan(const ssa_gconv_desc* d, size_t* ws_bytes);
int ssa_gconv3x3_bwd(const ssa_gconv_desc* d, const void* x, const void* dy, int lddy, const float* w, void* dx,
                     int lddx, float* dw, int accumulate, void* ws, void* stream);

/* ----------------------------------------------- rectangular-dilation 3x3 conv ----
 * nn.Conv2d(Cin, Cout, 3, stride = 1, padding = (dil_h, dil_w), dilation = (dil_h, dil_w), bias = False): the five convs
 * of the Dense Prediction Cell (dpc_conv / DPC, network/utils.py:249-260; rates (1,6) (18,15) (6,21) (1,1) (6,3), doubled at
 * output stride 8).  ssa_conv_desc has one dilation; this family has a descriptor and entry points of its own
 * (csrc/conv_dil.hip).  NHWC 16-bit, fp32 accumulate on MFMA.  x [B,H,W,Cin] with pixel stride ldx >= Cin, y [B,H,W,Cout]
 * with ldy >= Cout, both strides % 8, both pointers 16-byte aligned: x and y may be disjoint channel slices of ONE
 * allocation (the cell's convs write their slices of the concatenated output and read `a` back out of it).
 * Supported: Cin % 64 == 0 and Cout % 64 == 0, any B, H, W >= 1, any dil_h, dil_w >= 1 (dil >= H or W included: the
 * off-centre taps of that axis are then outside everywhere).  Other channel counts: SSA_EUNSUPPORTED (-2).  A bad
 * descriptor (NULL, B / H / W / Cin / Cout < 1, dil < 1, ldx < Cin, ldy < Cout, a stride % 8 != 0, 2^31 pixels or more)
 * or a NULL / misaligned operand: SSA_EINVAL (-1).  Nothing is launched in either case.
 * A tap reads zero wherever iy = oy + (kh-1) dil_h or ix = ox + (kw-1) dil_w leaves [0,H) x [0,W) of its own image; a
 * tap that is outside for a workgroup's whole 64-pixel tile costs that workgroup nothing.                          */
typedef struct ssa_dilconv_desc {
  int B, H, W, Cin, ldx;   /* x [B,H,W,Cin], pixel stride ldx   */
  int Cout, ldy;           /* y [B,H,W,Cout], pixel stride ldy  */
  int dil_h, dil_w;        /* dilation = padding, per axis      */
} ssa_dilconv_desc;
int ssa_dilconv3x3_supported(const ssa_dilconv_desc* d);
/* Forward, 16-bit output.  w_frag: ssa_pack_filter mode 2 of the OIHW parameter (cin_pad = Cin, Kpad = 9 Cin).  stats
 * (optional): the BatchNorm partial sums of the ROUNDED outputs with ssa_conv2d_tile's contract --
 * [ssa_bn_stat_replicas()][2][Cout] fp64, ACCUMULATED (caller clears).
 * DATA GRADIENT: with stride 1 and padding = dilation on both axes the data gradient is the same conv with the
 * flipped, transposed filter, so this entry point serves both: x = dy [B,H,W,Cout_fwd], y = dx [B,H,W,Cin_fwd], the
 * descriptor's Cin / Cout exchanged, w_frag = ssa_pack_filter mode 3 (cout_pad = Cout_fwd, Kpad = 9 Cout_fwd), stats NULL.
 * Group-aware: inside an ssa_group bracket several problems (the cell's b, c, d; their three data gradients) share
 * one launch.                                                                                                       */
int ssa_dilconv3x3(const ssa_dilconv_desc* d, const void* x, const void* w_frag, void* y, double* stats, void* stream);
/* Weight gradient: dw [Cout][Cin][3][3] fp32 (the parameter's OIHW layout) = sum over pixels of dy x; overwritten, or
 * added to when accumulate != 0 (dw = the layer's slice of the step's gradient arena, ssa_gconv3x3_bwd's rule).  x as in
 * the descriptor; dy [B,H,W,Cout] with pixel stride lddy (the descriptor's ldy is not read).  The sum over pixels has
 * a fixed order: workgroups split the pixel axis into *nsplit parts, write fp32 partials to ws (*ws_bytes of the plan,
 * 16-byte aligned, every byte of it overwritten) and a second launch adds the parts in order -- no floating-point
 * atomics.  Not group-aware (two dependent launches).                                                            */
int ssa_dilconv3x3_wgrad_plan(const ssa_dilconv_desc* d, int* nsplit, size_t* ws_bytes);
int ssa_dilconv3x3_wgrad(const ssa_dilconv_desc* d, const void* x, const void* dy, int lddy, float* dw, int accumulate,
                         void* ws, void* stream);

/* ------------------------------------------------- squeeze-and-excitation gate ----
 * z = relu(se_module(y) + residual), se_module(y) = y * sigmoid(fc2(relu(fc1(avg_pool(y))))): SEModule.forward and the
 * tail of Bottleneck.forward (network/SEresnext.py:84-91, 115-116).  y, r, z, dz, dy, dr: NHWC 16-bit [B,HW,C] with
 * pixel strides % 8 == 0 and >= C, 16-byte aligned, C % 8 == 0.  The gate reads the fp32 parameters in their own
 * storage -- w1 [Cr][C], b1 [Cr], w2 [C][Cr], b2 [C] (fc1 / fc2 are 1x1 convs) -- and all of its arithmetic is fp32;
 * mean [B][C], h [B][Cr], s [B][C], ds, g [B][C] are fp32.  Every sum has a fixed order (no atomics).  ws: ssa_se_plan's
 * bytes, one size for all entry points of a (B, HW, C, Cr).  A bad argument returns -1, Cr > min(C, 1024) -2, before
 * the device is touched.                                                                                          */
int ssa_se_plan(int B, long HW, int C, int Cr, size_t* ws_bytes);
/* squeeze + gate (replaces avg_pool, fc1, relu, fc2, sigmoid: SEresnext.py:86-90): mean = sum_p y / HW, summed by as
 * many workgroups as fill the chip; h = relu(W1 mean + b1); s = 1 / (1 + exp(-(W2 h + b2))).                      */
int ssa_se_squeeze_gate(const void* y, int ldy, int B, long HW, int C, int Cr, const float* w1, const float* b1,
                        const float* w2, const float* b2, float* mean, float* h, float* s, void* ws, void* stream);
/* apply (replaces `module_input * x`, `+ residual` and `self.relu`: SEresnext.py:91, 115-116):
 * z = round16(act(fma(s[b,c], y, r))); r nullable (no residual), the ReLU only if relu != 0.                     */
int ssa_se_apply(const void* y, int ldy, const void* r, int ldr, const float* s, void* z, int ldz, int B, long HW, int C,
                 int relu, void* stream);
/* backward, pass 1 over dz: ds[b,c] = sum_p m dz y, m = (z > 0) with relu != 0 (z then required), else 1.         */
int ssa_se_bwd_reduce(const void* dz, int lddz, const void* z, int ldz, const void* y, int ldy, int B, long HW, int C,
                      int relu, float* ds, void* ws, void* stream);
/* gate backward: a2 = ds s (1 - s); db2 = sum_b a2; dw2 = sum_b a2 h^T; a1 = (W2^T a2) (h > 0); db1 = sum_b a1;
 * dw1 = sum_b a1 mean^T; g = (W1^T a1) / HW -- the gradients are written, or added to when accumulate != 0.       */
int ssa_se_gate_bwd(const float* ds, const float* s, const float* h, const float* mean, const float* w1, const float* w2,
                    int B, long HW, int C, int Cr, float* g, float* dw1, float* db1, float* dw2, float* db2, int accumulate,
                    void* ws, void* stream);
/* backward, pass 2 over dz: dy = round16(fma(s[b,c], m dz, g[b,c])), dr = round16(m dz) (dr nullable).            */
int ssa_se_apply_bwd(const void* dz, int lddz, const void* z, int ldz, const float* s, const float* g, int B, long HW, int C,
                     int relu, void* dy, int lddy, void* dr, int lddr, void* stream);

/* ------------------------------------------------------- depthwise 3x3 conv ----
 * nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups = C, bias = False), the first half of every
 * SeparableConv2d of the Xception-71 trunk (network/xception.py:30-32; fixed_padding is symmetric for a 3x3 kernel).
 * NHWC 16-bit, C % 8 == 0, pixel strides % 8 and >= C, 16-byte aligned operands; w = the parameter's own
 * [C][1][3][3] fp32 storage.  A bad descriptor returns -1 before the device is touched.                        */
typedef struct ssa_dwconv_desc {
  int B, H, W, C, ldx;     /* x [B,H,W,C] */
  int Ho, Wo, ldy;         /* y [B,Ho,Wo,C], Ho = (H-1)/stride + 1 */
  int stride, dil;         /* stride 1 with dil >= 1, or stride 2 with dil 1; padding = dil */
} ssa_dwconv_desc;
/* y = round16(sum_taps w x).  stats (training; replaces the ssa_bn_stats pass of `self.bn`, xception.py:33,38):
 * sum y and sum y^2 of the values AS STORED are added into [ssa_bn_stat_replicas()][2][C] fp64 (caller clears).
 * coef (inference; replaces `self.bn` itself): rows 0 / 1 of the layer's [4][C] table, z = round16(scale * y + shift)
 * on the rounded y, then the ReLU if relu != 0 -- ssa_bn_apply on the stored y bit for bit.  Both: SSA_EUNSUPPORTED. */
int ssa_dwconv3x3(const ssa_dwconv_desc* d, const void* x, const float* w, void* y, double* stats,
                  const float* coef, int relu, void* stream);
/* Backward of the same conv (cuDNN's backward-data and backward-filter behind the grouped nn.Conv2d) in one pass over
 * dy and x: dx (nullable) [B,H,W,C] 16-bit, every pixel written; dw (nullable) [C][9] fp32, added to when accumulate
 * != 0.  ws: ssa_dwconv3x3_bwd_plan's bytes of workspace (the workgroups' fp32 partial sums of dw; needed with dw). */
int ssa_dwconv3x3_bwd_plan(const ssa_dwconv_desc* d, size_t* ws_bytes);
int ssa_dwconv3x3_bwd(const ssa_dwconv_desc* d, const void* x, const void* dy, int lddy, const float* w,
                      void* dx, int lddx, float* dw, int accumulate, void* ws, void* stream);

/* Label-map resize, mask.resize(size, Image.NEAREST) of
 * transforms/joint_transforms.py:193,267,290,319,339,364,466:
 * uint8 [B,Hs,Ws] -> [B,Hd,Wd], dst[y,x] = src[iy_table[y], ix_table[x]].  The
 * index tables carry Pillow's exact rule (a running double-precision sum, see
 * semseg_amd/datasets/transforms.py); the result is bit-identical to PIL.      */
int ssa_resize_nearest_u8(const unsigned char* src, int B, int Hs, int Ws,
                          unsigned char* dst, int Hd, int Wd, const int* iy_table,
                          const int* ix_table, void* stream);

/* ------------------------------------------------------------------- OCR ----
 * SpatialGather_Module.forward, network/ocr_utils.py:34-46 (K9) and
 * ObjectAttentionBlock.forward, network/ocr_utils.py:95-119 (K10).
 * The matrix products (probs^T @ feats, q @ k^T, sim @ v and their gradients)
 * run on ssa_conv2d_igemm / ssa_conv2d_wgrad as 1x1 GEMMs whose "filters" are
 * activations packed by ssa_pack_matrix; the functions below are the two
 * softmaxes and their backward.
 *
 * softmax over HW, per (image, class): logits fp32 [HW, K] (pixel stride ld);
 * rowstat fp32 [K][2] = (max, sum exp).                                       */
int ssa_softmax_hw_stats(const float* logits, int ld, long HW, int K,
                         float* rowstat, void* stream);
/* probs bf16 [HW, Kpad] (zero padded columns K..Kpad)                         */
int ssa_softmax_hw_probs(const float* logits, int ld, long HW, int K,
                         const float* rowstat, void* probs, int Kpad, void* stream);
/* out[k] = sum_c a[k,c]*b[k,c]                                                */
int ssa_rowdot_f32(const float* a, const float* b, int K, int C, float* out,
                   void* stream);
/* dlogits[p,k] (+)= probs[p,k] * (dprobs[p,k] - dot[k])                        */
int ssa_softmax_hw_bwd(const float* logits, int ld, long HW, int K,
                       const float* rowstat, const float* dprobs, int lddp,
                       const float* dot, float* dlogits, int lddl, int accumulate,
                       void* stream);
/* per-pixel softmax over K object regions of scale*sim: sim fp32 [P, K];
 * probs bf16 [P, Kpad]; backward returns dsim as bf16 [P, Kpad].              */
int ssa_softmax_lastdim_fwd(const float* sim, int ld, long P, int K, float scale,
                            void* probs, int Kpad, void* stream);
int ssa_softmax_lastdim_bwd(const float* sim, int ld, long P, int K, float scale,
                            const float* dprobs, int lddp, void* dsim, int Kpad,
                            void* stream);
/* GEMM operand from an activation matrix: dst bf16 [rows_out][Kpad] = src
 * (or src^T), zero padded.  src_dtype 0 bf16, 1 fp32; src is [R][C], row
 * stride ld.                                                                  */
int ssa_pack_matrix(const void* src, int src_dtype, int R, int C, int ld,
                    int transpose, void* dst, int rows_out, int Kpad, void* stream);

/* Fused object attention (network/ocr_utils.py:100-113; csrc/ocr_attn.hip): out[p, :] = softmax_K(scale * q[p, :] k^T) v
 * per image, one launch, sim / probs never leave the registers.  q: [P] pixel rows of Dch = 256 16-bit channels with
 * pixel stride ldq, k / v: dense [K][256] 16-bit, out: [P] rows with stride ldo.  K <= 96 object regions
 * (ssa_ocr_attn_supported; otherwise the caller runs the three-launch form on ssa_conv2d_igemm +
 * ssa_softmax_lastdim_*).  Group-aware (the scale passes of a step share one launch).
 * Backward: dq, and the two [P][Kpad] 16-bit matrices (Kpad = K rounded up to 32, padding = 0) the pixel reductions
 * dv = probs^T dout and dk = dsim^T q are computed from (ssa_conv2d_wgrad with KH = KW = 1):
 * probs = the forward's probabilities, dsim = scale * probs * (dprobs - <probs, dprobs>), dprobs = dout v^T.          */
int ssa_ocr_attn_supported(int K, int Dch);
int ssa_ocr_attn_fwd(const void* q, int ldq, const void* k, const void* v, long P, int K, int Dch, float scale,
                     void* out, int ldo, void* stream);
int ssa_ocr_attn_bwd(const void* q, int ldq, const void* k, const void* v, const void* dout, int lddo, long P, int K,
                     int Dch, float scale, void* dq, int lddq, void* probs, void* dsim, void* stream);

/* ----------------------------------------------------- scale attention -----
 * sigmoid of the attention logit (network/utils.py:363) and the two-scale
 * fusion of MscaleOCR.two_scale_forward, network/ocrnet.py:289-298 (K11):
 *   joint = up(attn*p_lo) + (1 - up(attn)) * p_hi   (all fp32 NHWC)           */
int ssa_sigmoid_fwd(const float* x, float* y, long n, void* stream);
int ssa_sigmoid_bwd(const float* y, const float* dy, float* dx, long n, void* stream);
/* out[p,c] = a[p]*x[p,c]  (attn broadcast over classes), and its backward.   */
int ssa_bcast_mul_fwd(const float* a, const float* x, float* out, long P, int C,
                      void* stream);
int ssa_bcast_mul_bwd(const float* a, const float* x, const float* dout, float* da,
                      float* dx, long P, int C, void* stream);
/* joint[p,c] = lo[p,c] + (1-a[p])*hi[p,c], and its backward.                  */
int ssa_attn_blend_fwd(const float* lo, const float* a, const float* hi,
                       float* joint, long P, int C, void* stream);
int ssa_attn_blend_bwd(const float* a, const float* hi, const float* djoint,
                       float* da, float* dhi, long P, int C, int accumulate_da,
                       void* stream);

/* ---------------------------------------------------------------- losses ----
 * CrossEntropyLoss2d, loss/utils.py:121-134 (K13): mean over valid pixels of
 * -log_softmax(x)[t], ignore_index skipped.  logits fp32 NHWC [P,C], labels
 * int64 [P].  acc = {sum nll, valid count} fp64; dlogits (optional) receives
 * softmax - onehot for valid pixels (un-normalised; scale in ssa_scale_grad).  */
int ssa_ce_fwd(const float* logits, int ld, const int64_t* labels, long P, int C,
               int ignore_index, double* acc, float* dlogits, void* stream);
/* RMILoss.forward_sigmoid part I, loss/rmi.py:91-116 (K14): masked BCE with
 * logits, sum over pixels and classes; acc = {sum bce, valid count}.
 * dlogits = (sigmoid(x) - onehot) * mask (un-normalised).                     */
int ssa_bce_fwd(const float* logits, int ld, const int64_t* labels, long P, int C,
                double* acc, float* dlogits, void* stream);
/* loss = acc[0] / (acc[1] + denom_add) ; writes fp32 scalar                    */
int ssa_loss_finalize(const double* acc, double denom_add, float* loss, void* stream);
/* g[i] *= upstream[0] * coef / (acc[1] + denom_add); g = 0 when that
 * denominator is 0 (cross entropy over fully ignored labels: torch's gradient) */
/* Backward of ssa_bce_fwd WITHOUT its saved gradient: dlogits = (sigmoid - onehot) * mask * upstream * coef /
 * (acc[1] + denom_add), recomputed from the logits (dense [P, C], ld == C, P * C % 4 == 0, 16-byte aligned; otherwise
 * SSA_EUNSUPPORTED and the caller scales the gradient ssa_bce_fwd saved).  loss/rmi.py:103-112's autograd backward. */
int ssa_bce_bwd(const float* logits, int ld, const int64_t* labels, long P, int C, const float* upstream,
                double coef, const double* acc, double denom_add, float* dlogits, void* stream);
int ssa_scale_grad(float* g, long n, const float* upstream, double coef,
                   const double* acc, double denom_add, void* stream);
/* dst[i] = src[i] * upstream[0] * coef / (acc[1] + denom_add): the same without touching src (the un-normalised
 * gradient the forward saved stays valid; the backward needs no copy of it)       */
int ssa_scale_grad_to(const float* src, float* dst, long n, const float* upstream, double coef,
                      const double* acc, double denom_add, void* stream);

/* RMILoss.rmi_lower_bound, loss/rmi.py:139-215 + loss/rmi_utils.py:15-56,
 * 95-107 (K15).  Fused: sigmoid*mask+1e-6 -> 4x4/4 avg pool (pad 2) ->
 * 3x3-neighbourhood Gram matrices in fp64 (never materialising the
 * [B,C,9,65025] stack) -> 9x9 inverse / Cholesky per (b,c) in one wavefront.
 * ssa_rmi_pool: 1 <= C <= 128 classes (the limit of ssa_ce_fwd / ssa_bce_fwd),
 * ld >= C; above 30 classes the workgroups take the classes in chunks of <= 30
 * (LDS stays within 64 KB).  Labels outside [0, C) are ignored (label == C
 * included: Mapillary's ignore label 65).                                    */
int ssa_rmi_pool(const float* logits, int ld, const int64_t* labels, int B, int H,
                 int W, int C, float* pooled_pr, float* pooled_la, int Hp, int Wp,
                 void* stream);
int ssa_rmi_gram(const float* pooled_pr, const float* pooled_la, int BC, int Hp,
                 int Wp, double* gram /*[BC][189]*/, void* stream);
/* per (b,c): loss value + gradient matrices G_lp, G_pp (9x9) + means.         */
int ssa_rmi_solve(const double* gram, int BC, int Hp, int Wp, double* loss_bc,
                  double* gmat /*[BC][2*81+18]*/, void* stream);
/* rmi = sum_c mean_b loss_bc / 9  -> fp32 scalar                              */
int ssa_rmi_finalize(const double* loss_bc, int B, int C, float* out, void* stream);
/* d rmi / d pooled_pr  [BC][Hp][Wp] fp32                                      */
int ssa_rmi_bwd_pooled(const float* pooled_pr, const float* pooled_la,
                       const double* gmat, int BC, int Hp, int Wp, float* dpooled,
                       void* stream);
/* dlogits[p,c] += coef*upstream * dpooled[cell(p)]/16 * mask * s*(1-s)        */
int ssa_rmi_bwd_logits(const float* logits, int ld, const int64_t* labels, int B,
                       int H, int W, int C, const float* dpooled, int Hp, int Wp,
                       const float* upstream, double coef, float* dlogits,
                       int accumulate, void* stream);
/* The same with the BCE half of RMILoss.forward_sigmoid's gradient (loss/rmi.py:103-134: 0.5 * bce + 0.5 * rmi) folded in:
 * dlogits = bce_grad * upstream * bce_coef / (bce_acc[1] + bce_denom_add) + the RMI term -- what ssa_scale_grad_to
 * followed by the accumulating form computes, in one pass over the logits' gradient.  bce_grad NULL: the BCE half is
 * recomputed from the logits (the forward then saves no gradient).                                                */
int ssa_rmi_bwd_logits_bce(const float* logits, int ld, const int64_t* labels, int B, int H, int W, int C,
                           const float* dpooled, int Hp, int Wp, const float* upstream, double coef,
                           const float* bce_grad, double bce_coef, const double* bce_acc, double bce_denom_add,
                           float* dlogits, void* stream);

/* Label relaxation (--jointwtborder): ImgWtLossSoftNLL, loss/utils.py:150-231, on the target of
 * RelaxedBoundaryLossToTensor, transforms/transforms.py:74-123 (K16).  The [C+1,H,W] multi-hot target never exists
 * on the training path: a pixel's class SET is two 64-bit words, sets[p][2], bit c = class c, bit C = the ignore
 * channel (1 <= C <= 127, otherwise SSA_EUNSUPPORTED).  stats is int64 [B][C+2] per image: the number of set entries
 * of each of the C+1 channels (what calculate_weights sums, loss/utils.py:165-177), then the number of pixels whose
 * set holds no real class (`ignore_mask`, loss/utils.py:212).  Integer sums: exact, whatever the order.
 *
 * ssa_relax_mask_labels: transforms/transforms.py:90-117.  labels [B][H][W], int64 or (label_u8) uint8; a label equal
 * to ignore_index or outside [0, C) is class C (the rule of ssa_rmi_pool); the set of a pixel is the union of the
 * labels of its (2*border+1)^2 window, positions outside the image counting as C (`shift(..., cval=num_classes)`);
 * border 0, 1 or 2 (cfg.BORDER_WINDOW), otherwise SSA_EUNSUPPORTED.  strict_lo/strict_hi: cfg.STRICTBORDERCLASS as a
 * bit set (0, 0 = None): a pixel whose own label is in it keeps the one-hot of that label (transforms.py:95-99,114).
 * Clears stats itself, by a small launch in front of the kernel.                                                    */
int ssa_relax_mask_labels(const void* labels, int label_u8, int B, int H, int W, int C, int ignore_index, int border,
                          unsigned long long strict_lo, unsigned long long strict_hi, unsigned long long* sets,
                          int64_t* stats, void* stream);
/* The same from the reference's own target, uint8 [B][C+1][H][W], non-zero = set (loss/utils.py:207-213).         */
int ssa_relax_mask_multihot(const unsigned char* multihot, int B, int H, int W, int C, unsigned long long* sets,
                            int64_t* stats, void* stream);
/* sets -> uint8 [B][C+1][H][W] of 0 / 1: what RelaxedBoundaryLossToTensor.__call__ returns (transforms.py:117-123). */
int ssa_relax_multihot(const unsigned long long* sets, int B, int H, int W, int C, unsigned char* out, void* stream);
/* calculate_weights, loss/utils.py:165-177, and `torch.Tensor(class_weights)` of :227: w[B][C] fp32 =
 * (float)((hist != 0) * upper_bound * (1 - hist) + 1) with hist = count / total in fp64, total over all C+1 channels;
 * batch_weights (cfg.BATCH_WEIGHTING, :218-219): the counts summed over the batch first, every row the same.
 * Also zeroes acc[B], the accumulators of ssa_relax_nll_fwd.                                                       */
int ssa_relax_weights(const int64_t* stats, int B, int C, double upper_bound, int batch_weights, float* w,
                      double* acc, void* stream);
/* custom_nll, loss/utils.py:179-205, per image i over its H*W pixels: acc[i] += -q[p] * (sum_{c in set} w[i][c]) *
 * log(sum_{c in set} softmax(x)[c]), 0 where the set holds no real class;  q[p] = sum_b 1 / max(1, |set_b[p]|) over
 * ALL images of the batch (`border_weights` is passed whole at :228 and broadcasts at :196).  logits fp32 NHWC
 * [B*H*W][C] with leading dimension ld >= C.  acc must be zero (ssa_relax_weights).                               */
int ssa_relax_nll_fwd(const float* logits, int ld, const unsigned long long* sets, const float* w, int B, int H, int W,
                      int C, double* acc, void* stream);
/* loss = sum_i acc[i] / (H*W - stats[i][C+1] + 1)  (loss/utils.py:203-204,229) -> fp32 scalar                     */
int ssa_relax_nll_finalize(const double* acc, const int64_t* stats, int B, int H, int W, int C, float* loss,
                           void* stream);
/* Backward of the two above, recomputed from the logits (as ssa_bce_bwd): dlogits dense [B*H*W][C] =
 * upstream[0] / (H*W - stats[i][C+1] + 1) * q * (sum_{c in set} w[i][c]) * (softmax[k] - [k in set] softmax[k] / S). */
int ssa_relax_nll_bwd(const float* logits, int ld, const unsigned long long* sets, const float* w, const int64_t* stats,
                      int B, int H, int W, int C, const float* upstream, float* dlogits, void* stream);

/* Boundary F-score: eval_mask_boundary, utils/f_boundary.py:61-92, over db_eval_boundary (:110-173) and the full-size
 * branch of seg2bmap (:175-233), for every class of every image in two launches.  pred_u8 [B][H][W] uint8 (the `pred`
 * bytes of ssa_eval_tail), gts [B][H][W] int64 or (gts_u8) uint8.  A pixel whose ground truth equals ignore_label is
 * cleared in BOTH maps (:133-134); a ground-truth label outside [0, C) that is not ignore_label, and a prediction byte
 * >= C, belong to no class.  Class c is a boundary class of a pixel iff c occurs in its 2 x 2 quad {p, e, s, se} and
 * not every member is c (:209-217); on the last row the quad is the pair {p, e}, on the last column {p, s}, and the
 * bottom-right pixel is no boundary (:218-220).  radius = disk(bound_pix) of :127-128,142-143 as an integer, taken by
 * the host: a boundary pixel is matched iff the other map has a boundary pixel of its class at dx^2 + dy^2 <=
 * radius^2, positions outside the image being empty.
 * counts int64 [B][C][4] = {n_fg, n_gt, fg_match, gt_match} (:146-151,164-165), cleared by the first launch: exact
 * integer sums.  Precision, recall and F (:154-171) are the host's, in float64.
 * workspace: 8 * B * H * W bytes (ssa_fboundary_workspace_bytes), 4-byte aligned: both boundary maps as four class
 * bytes per pixel, 0xFF = empty.  1 <= C <= 254 and 0 <= radius <= 32, otherwise SSA_EUNSUPPORTED; B <= 65535.      */
int ssa_fboundary_workspace_bytes(int B, int H, int W, size_t* bytes);
int ssa_fboundary_counts(const unsigned char* pred_u8, const void* gts, int gts_u8, int B, int H, int W, int C,
                         int ignore_label, int radius, int64_t* counts, void* workspace, size_t workspace_bytes,
                         void* stream);

/* Tail of the input pipeline on the device: joint crop window + optional
 * horizontal flip of the cropped pair (transforms/joint_transforms.py:276-281
 * RandomHorizontallyFlip after the crop transforms), then for the image ToTensor + Normalize
 * (datasets/base_loader.py:141-142; mean/std of config.py:96-97) written as the NHWC bf16
 * [ch][cw][cpad] tensor the trunk reads (channels 3.. zero), value
 * bf16(((float)u8/255 - mean[c]) / std[c]) in IEEE fp32 -- bit-identical to the CPU transforms
 * followed by .to(bfloat16); for the labels MaskToTensor (uint8 -> int64).
 * img_hwc: uint8 [H][W][3] RGB on the device; lab_hw: uint8 [H][W].  mean3/std3: HOST floats.  */
int ssa_image_u8_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0,
                                     int cw, int ch, int flip, const float* mean3,
                                     const float* std3, void* out_nhwc_bf16, int cpad,
                                     void* stream);
int ssa_label_u8_crop_flip(const unsigned char* lab_hw, int H, int W, int x0, int y0, int cw,
                           int ch, int flip, int64_t* out, void* stream);

/* The scale step of the input pipeline on the device:
 * `img.resize((w, h), Image.BICUBIC)` of transforms/joint_transforms.py:433-471 (RandomSizeAndCrop ->
 * scale_and_crop; also the Scale / ResizeHeight transforms) is Pillow's two-pass 8-bit resampling
 * (libImaging/Resample.c): a horizontal pass into an 8-bit image, then a vertical pass over it.  One
 * call = one pass over an interleaved uint8 [Hs][Ws][C] device image along axis 1 (x: n_out output
 * columns) or 0 (y: n_out output rows); bounds [n_out][2] = (first source index, tap count) and coefs
 * [n_out][ksize] = 22-bit fixed-point taps are DEVICE arrays the host derives exactly as
 * precompute_coeffs / normalize_coeffs_8bpc do (semseg_amd/datasets/transforms.py).  Integer
 * arithmetic: bit-identical to Pillow.                                                          */
int ssa_resample_u8(const unsigned char* src, int Hs, int Ws, int C, int axis, unsigned char* dst,
                    int n_out, const int* bounds, const int* coefs, int ksize, void* stream);

/* ColorJitter on the device (transforms/transforms.py:192-362; built as ColorJitter(0.25, 0.25, 0.25, 0.25)
 * by datasets/__init__.py:94-99 under the default --color_aug): the image-only augmentation between the joint
 * crop / flip and ToTensor + Normalize, bit-identical to Pillow's ImageEnhance.Brightness / Contrast / Color
 * and to the HSV round trip of adjust_hue (csrc/color_jitter.hip states the arithmetic).
 * A program is up to four DISTINCT steps in application order (the order ColorJitter.get_params shuffled);
 * factor[] is indexed by the op code of the three blend steps, hue_byte = trunc(hue_factor * 255) mod 256 is
 * added to H.  It is a HOST struct: the entry points pass it to the kernels by value.                    */
enum { SSA_JITTER_BRIGHTNESS = 0, SSA_JITTER_CONTRAST = 1, SSA_JITTER_SATURATION = 2, SSA_JITTER_HUE = 3 };
typedef struct ssa_jitter_program {
  int n_ops;        /* 0..4 */
  int op[4];        /* SSA_JITTER_* */
  float factor[3];  /* brightness, contrast, saturation */
  int hue_byte;     /* 0..255 */
} ssa_jitter_program;

/* transforms/transforms.py:192-362, datasets/__init__.py:94-99 -- the sum ImageEnhance.Contrast averages:
 * *counter = sum over the window (x0, y0, cw, ch) of img_hwc (uint8 [H][W][3] on the device) of
 * L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of the pixel AFTER the steps that precede the program's
 * contrast step.  counter: one 8-byte-aligned 64-bit DEVICE word, cleared here on the stream (by a one-thread launch).  Integer
 * addition: exact and independent of the order.  A program without a contrast step launches nothing (counter
 * may then be NULL).                                                                                      */
int ssa_jitter_luma_sum(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                        const ssa_jitter_program* program, unsigned long long* counter, void* stream);
/* transforms/transforms.py:192-362, datasets/__init__.py:94-99 -- the whole program on the window, optionally
 * mirrored (the contrast mean does not change under the flip): out_hwc uint8 [ch][cw][3] on the device.  The
 * contrast mean m = int(*counter / (cw * ch) + 0.5) is formed ON THE DEVICE from what ssa_jitter_luma_sum
 * left (same window, same program, same stream): no host synchronisation between the two.               */
int ssa_jitter_apply_u8(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch, int flip,
                        const ssa_jitter_program* program, const unsigned long long* counter,
                        unsigned char* out_hwc, void* stream);
/* transforms/transforms.py:192-362, datasets/__init__.py:94-99 followed by ToTensor + Normalize
 * (datasets/__init__.py:104-107): ssa_jitter_apply_u8 fused with the arithmetic and the NHWC [ch][cw][cpad]
 * store of ssa_image_u8_crop_flip_normalize, in the build's 16-bit element type.  Bit-identical to the two in
 * sequence.  All three return -1 before touching the device on a bad window, an unknown or repeated op code,
 * a null pointer, or a program with a contrast step and no counter.                                       */
int ssa_jitter_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                                   int flip, const ssa_jitter_program* program,
                                   const unsigned long long* counter, const float* mean3, const float* std3,
                                   void* out_nhwc_bf16, int cpad, void* stream);

/* RandomGaussianBlur on the device (transforms/transforms.py:154-162; datasets/__init__.py:102 appends it under
 * --gblur): skimage.filters.gaussian(img, sigma, multichannel=True) * 255 truncated to uint8, i.e. the bytes as
 * float64 (x * (1 / 255): the 256-entry table lut256), scipy.ndimage.gaussian_filter(., [sigma, sigma, 0],
 * mode='nearest', truncate=4.0), bit for bit (csrc/gblur.hip states the arithmetic).  The taps are a HOST struct,
 * passed to the kernel by value: radius = int(4 sigma + 0.5) in 1..5 -- the reference's whole interval of sigma,
 * [0.15, 1.3) --, w[j] the normalised weight at distance j (w[j] for j > radius is not read, but must be finite). */
typedef struct ssa_gblur_taps {
  int radius;   /* 1..5 */
  double w[6];  /* w[0] centre ... w[radius] */
} ssa_gblur_taps;

/* transforms/transforms.py:154-162, datasets/__init__.py:102 -- the blur of the window (x0, y0, cw, ch) of img_hwc
 * (uint8 [H][W][3] on the device), optionally mirrored: out_hwc uint8 [ch][cw][3].  Indices beyond the WINDOW's
 * edges are clamped to the window, not to the source image: the reference blurs the cropped image.  program: NULL, or
 * the ColorJitter program to run on every pixel before the blur (the reference's order); a program with a contrast
 * step reads the mean from `counter` as ssa_jitter_luma_sum left it (same window, same program, same stream; no
 * host synchronisation).  lut256: 256 doubles on the DEVICE, lut256[b] = the float64 the reference makes of byte b. */
int ssa_gblur_u8(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch, int flip,
                 const ssa_jitter_program* program, const unsigned long long* counter,
                 const ssa_gblur_taps* taps, const double* lut256, unsigned char* out_hwc, void* stream);
/* transforms/transforms.py:154-162, datasets/__init__.py:102 followed by ToTensor + Normalize
 * (datasets/__init__.py:104-107): ssa_gblur_u8 fused with the arithmetic and the NHWC [ch][cw][cpad] store of
 * ssa_image_u8_crop_flip_normalize, in the build's 16-bit element type; cpad must be 16.  Bit-identical to the two in
 * sequence.  Both return -1 before touching the device on a bad window, a radius outside 1..5, a null pointer, a cpad
 * other than 16, an invalid program, or a program with a contrast step and no counter.                      */
int ssa_gblur_crop_flip_normalize(const unsigned char* img_hwc, int H, int W, int x0, int y0, int cw, int ch,
                                  int flip, const ssa_jitter_program* program,
                                  const unsigned long long* counter, const ssa_gblur_taps* taps,
                                  const double* lut256, const float* mean3, const float* std3, void* out_nhwc,
                                  int cpad, void* stream);

/* RandAugment on the device (datasets/randaugment.py: RandAugment 250-263, augment_list 179-201, affine_transform
 * 16-22, the operations 25-142; datasets/__init__.py:83-87 applies it under --rand_augment N,M to the cropped and
 * mirrored pair, before ColorJitter): the 14 operations of augment_list, each bit-identical to the Pillow call the
 * reference makes (csrc/randaugment.hip states the arithmetic).  The op codes are the indices of augment_list.
 * A program is the drawn chain in application order.  value[k] is the SIGNED value the operation was called with, after
 * its own sign draw: the shear (ShearX 25-29, ShearY 32-36), the translation in pixels (TranslateX 39-45, TranslateY
 * 48-54), the angle in degrees (Rotate 71-78), the Solarize threshold (101-104), the Posterize bits 4..8 (107-111), the
 * blend factor of Color, Brightness, Sharpness (127-142); unused by Identity (175-176), AutoContrast (81-83), Invert
 * (86-88), Equalize (91-93).  matrix[k] holds, for the five geometric operations, the six coefficients handed to
 * Image.transform(size, AFFINE, ...), prepared on the host in fp64 (Rotate: Image.rotate's rounded matrix about the
 * window's centre); a Rotate whose angle is a multiple of 360 degrees is a copy and its matrix is not read.
 * It is a HOST struct: the entry point reads it and passes each kernel its own small argument block by value. */
enum { SSA_RANDAUG_IDENTITY = 0, SSA_RANDAUG_SHEARX = 1, SSA_RANDAUG_SHEARY = 2, SSA_RANDAUG_TRANSLATEX = 3,
       SSA_RANDAUG_TRANSLATEY = 4, SSA_RANDAUG_ROTATE = 5, SSA_RANDAUG_AUTOCONTRAST = 6, SSA_RANDAUG_INVERT = 7,
       SSA_RANDAUG_EQUALIZE = 8, SSA_RANDAUG_SOLARIZE = 9, SSA_RANDAUG_POSTERIZE = 10, SSA_RANDAUG_COLOR = 11,
       SSA_RANDAUG_BRIGHTNESS = 12, SSA_RANDAUG_SHARPNESS = 13, SSA_RANDAUG_N_OPS = 14 };
#define SSA_RANDAUG_MAX_OPS 8
typedef struct ssa_randaug_program {
  int n_ops;                              /* 0..SSA_RANDAUG_MAX_OPS */
  int op[SSA_RANDAUG_MAX_OPS];            /* SSA_RANDAUG_* */
  double value[SSA_RANDAUG_MAX_OPS];
  double matrix[SSA_RANDAUG_MAX_OPS][6];
} ssa_randaug_program;

/* datasets/randaugment.py:256-263 (RandAugment.__call__ with the draws already made) on the window (x0, y0, cw, ch) of
 * img_hwc (uint8 [H][W][3] on the device) and of lab_hw (uint8 [H][W], or NULL: the image alone), mirrored first under
 * `flip`: img_out uint8 [ch][cw][3], lab_out uint8 [ch][cw].  Only the geometric operations touch the labels (NEAREST,
 * fill = ignore_label, the reference's fillmask); the image fill is (0, 0, 0).  img_tmp / lab_tmp: a second buffer of the
 * output's size, needed when more than one operation rewrites the image / the labels (the launches alternate between the
 * two; the last one writes the output).  hist: 768 uint32 per AutoContrast / Equalize of the program, ZEROED by the caller
 * in stream order; the tables of those two are derived from it on the device, so nothing here waits for the device or
 * reads from it, and the sequence can be captured into a graph.  Launches: one per operation on the image, one per
 * geometric operation on the labels, one histogram per AutoContrast / Equalize, and one crop / flip copy when no
 * operation rewrites the image or the labels.  Returns -1 before touching the device on a null image or output, an empty
 * or outside window, an op code outside 0..13, more than SSA_RANDAUG_MAX_OPS operations, Posterize bits outside 4..8, a
 * value or coefficient that is not finite, a missing buffer; -2 for a nearest-neighbour warp of a window larger than 8192
 * in either direction (Pillow's 16.16 sums leave its 32-bit integers there).  The outputs must not overlap the inputs. */
int ssa_randaug_u8(const unsigned char* img_hwc, const unsigned char* lab_hw, int H, int W, int x0, int y0, int cw,
                   int ch, int flip, const ssa_randaug_program* program, int ignore_label, unsigned int* hist,
                   unsigned char* img_out, unsigned char* img_tmp, unsigned char* lab_out, unsigned char* lab_tmp,
                   void* stream);

/* Class-uniform sampling (--class_uniform_pct, train.py:78, config.py:102): the centroid pass of
 * class_centroids_image, datasets/uniform.py:84-135, over N label maps of one size (csrc/centroids.hip).
 * labels: uint8 [N][H][ld] on the device, ld >= W.  Tiles are those of calc_tile_locations (uniform.py:67-81):
 * H / tile rows by W / tile columns of full tiles, y-major; pixels of the remainder count nowhere; an image smaller
 * than a tile has no tiles (nothing is launched, SSA_OK).  lut: NULL, or 256 bytes on the device applied to every
 * label as it is read -- the id2trainid step, uniform.py:112-121, which compares against the untouched copy of the
 * mask and is therefore a plain table.  1 <= C <= 256; a mapped label >= C (255 = ignore) counts nowhere.
 * sums: uint64 [N][tiles][C][3] = (pixels of the class in the tile, sum of their tile-local x, of their tile-local
 * y); cleared by a launch in front.  centroids: int32 [N][tiles][C][2] = (sum_x / n + x_offs, sum_y / n + y_offs)
 * by integer floor division -- what `int(center_of_mass(...))` gives, uniform.py:127-131 --, (-1, -1) where n == 0;
 * written by a finalize launch of the same call.  Integer sums: exact, whatever the order.  No host
 * synchronisation, no allocation; capturable.                                                                      */
int ssa_class_centroids_u8(const unsigned char* labels, int N, int H, int W, int ld, int tile, int C,
                           const unsigned char* lut, unsigned long long* sums, int* centroids, void* stream);

/* Constant padding of an image or a label map (csrc/pad_u8.hip): `ImageOps.expand(img, border, fill)` of
 * RandomCrop.__call__, transforms/joint_transforms.py:163-178, and add_margin, joint_transforms.py:48-60 (called at
 * 126-141), for RGB and L images.  src: uint8 [H][W][channels] on the device, channels 1 or 3; dst:
 * [H+top+bottom][W+left+right][channels]; fill: 3 HOST bytes (a label map takes the first).                       */
int ssa_pad_u8(const unsigned char* src, int H, int W, int channels, int left, int top, int right, int bottom,
               const unsigned char* fill, unsigned char* dst, void* stream);

/* The label half of the auto-labelled coarse data path (csrc/autolabel.hip), over N items of one size: what
 * BaseLoader.read_images and the thresholding of __getitem__ (datasets/base_loader.py:152-229; compare_current = 1) and
 * the id2trainid loop of class_centroids_image (datasets/uniform.py:104-121; compare_current = 0) make of an
 * auto-label map `labels`, the gtCoarse labelIds map `coarse` and the `_prob.png` map `prob`, uint8 [N][H][ld_*] on the
 * device, ld_* >= W.  With o = labels inside the window [win_x0, win_x1) x [win_y0, win_y1) and 0 outside it (the drop
 * mask, base_loader.py:59-60, 173-174; an EMPTY window, x1 <= x0 or y1 <= y0, means no drop mask), g = coarse and, per
 * image, mask = cmp = o:
 *     for (k, v, boost) in steps, in order:
 *         hit = (cmp == k)                         compare_current = 1: cmp IS mask, as rewritten so far
 *                                                  compare_current = 0: cmp stays the untouched o
 *         if boost and hit is non-empty in THIS image:  hit |= (g == k)
 *         mask[hit] = v
 *     out = prob < prob_cut ? ignore_label : mask          (prob_cut = 0: no threshold; the host forms
 *                                                           prob_cut = #{b in 0..255 : b / 255.0 < CUSTOM_COARSE_PROB})
 * steps: n_steps x (key, value, boost) HOST bytes, 0 <= n_steps <= 256 (0: the identity); they travel as kernel
 * arguments, so a captured call has them baked in.  coarse may be NULL when no step is boosted (g reads as 0), prob
 * when prob_cut == 0.  Workspaces on the device, both written before they are read: pairs, uint32 [N][2048], the
 * (o, g) pairs that occur in each image as a bit set; table, uint8 [N][65536], table[o][g] = the value of the pair after
 * the steps, written for the pairs that occur and for no other (the apply pass reads only those).  out: uint8 [N][H][ld_out], ld_out >= W; the bytes
 * between W and ld_out are not written.  The outputs must not overlap the inputs.  FOUR launches whatever the arguments
 * (clear, pair presence, resolve with one workgroup per image, apply), none when N * H * W == 0; no host synchronisation,
 * no allocation; capturable, and a replay follows the data.  Returns -1 before touching the device on a null labels /
 * pairs / table / out, a misaligned pairs, ld < W, n_steps outside 0..256, a boosted step without coarse, prob_cut
 * outside 0..256 or without prob, ignore_label outside 0..255, compare_current outside 0..1 and a non-empty window that
 * leaves the image.                                                                                                */
int ssa_autolabel_u8(const unsigned char* labels, const unsigned char* coarse, const unsigned char* prob, int N, int H,
                     int W, int ld_labels, int ld_coarse, int ld_prob, const unsigned char* steps, int n_steps,
                     int compare_current, int win_x0, int win_y0, int win_x1, int win_y1, int prob_cut, int ignore_label,
                     unsigned int* pairs, unsigned char* table, unsigned char* out, int ld_out, void* stream);

/* Evaluation tail on the device (utils/trnval_utils.py:173-196 + utils/misc.py:50-67
 * fast_hist): pred[p] = first argmax_c logits[p,c] (uint8, optional) and
 * hist[gt*C + pred] += 1 for 0 <= gt < C (int64 [C*C], ACCUMULATED: clear it once per
 * evaluation).  logits fp32 NHWC [P,C] (pixel stride ld), labels int64 [P].          */
int ssa_confusion_matrix(const float* logits, int ld, const int64_t* labels, long P, int C,
                         unsigned char* pred_out, int64_t* hist, void* stream);

/* The whole tail of eval_minibatch in one launch (utils/trnval_utils.py:116-196, utils/misc.py:50-67,
 * loss/utils.py:121-134; csrc/eval_tail.hip).  With the reference's statement order:
 *     out[p,c] = 0.0f;  for s in 0 .. n_src-1:  out[p,c] = out[p,c] + src_s[flips[s] ? mirror_w(p) : p, c]
 *     out[p,c] = (out[p,c] / div_scales) / div_flips                 two IEEE fp32 divisions, in this order
 *     m = max_c out[p,c];  arg = first c with out[p,c] == m  (a NaN wins once, as in ssa_confusion_matrix)
 *     se = sum_c exp(out[p,c] - m)
 *     pred[p] = arg                                   uint8 [P]            optional
 *     prob[p] = 1 / se  (= max_c softmax(out)[p])     fp32  [P]            optional
 *     err[p]  = gt >= 0 && gt != ignore_label && arg != gt    uint8 [P]    optional, needs labels
 *     hist[gt*C + arg] += 1  for 0 <= gt < C          int64 [C*C], ACCUMULATED   optional, needs labels
 *     loss_acc[0] += (m + log se) - out[p,gt];  loss_acc[1] += 1   for gt != ignore_label && 0 <= gt < C
 *                                                     double[2], ACCUMULATED (CrossEntropyLoss2d = [0] / [1])
 *     avg[p,c] = out[p,c]                             fp32 dense [P,C]     optional
 * srcs / flips: HOST arrays of n_src (1 .. 8) entries: device pointers to fp32 NHWC tensors [B,H,W,C] of common pixel
 * stride ld >= C, and "mirrored along W" flags (mirror_w(b,y,x) = (b,y,W-1-x): the flip is an index, never a tensor).
 * The pointers travel as kernel arguments.  labels int64 [B,H,W] or NULL.  1 <= C <= 128.  SSA_EINVAL (before the
 * device is touched) for anything else, for a null source, for an output that needs labels without labels and when
 * no output is asked for.                                                                                      */
int ssa_eval_tail(const float* const* srcs, const int* flips, int n_src, int ld, int B, int H, int W, int C,
                  const int64_t* labels, int ignore_label, float div_scales, float div_flips,
                  unsigned char* pred, float* prob, unsigned char* err, int64_t* hist, double* loss_acc,
                  float* avg, void* stream);

/* ImageDumper.dump on the device (utils/misc.py:279-386, driven from train.py:552-597; csrc/dump_tail.hip): one streaming
 * launch over the H x W pixels p of ONE image.  With u8(v) = v truncated toward zero to a byte,
 *     input_rgb[p][c] = u8(((image[c*plane_stride + p] - inv_mean3[c]) / inv_std3[c]) * 255.0f)
 *                                     torchvision's Normalize (sub_, div_) then ToPILImage (mul(255).byte()),
 *                                     misc.py:240-245, 326-329; inv_mean3 / inv_std3 are 3 HOST floats each, the fp32
 *                                     values the reference forms from -mean/std and 1/std; three fp32 operations each
 *                                     rounded on its own, a true IEEE division, no FMA
 *     gt_rgb[p]   = palette[gts[p] & 255]    the low 8 bits as in astype(np.uint8)      colorize_mask(..).convert('RGB'),
 *     pred_rgb[p] = palette[pred[p]]                                                      misc.py:333-341
 *     comp_rgb[p][c] = u8(a + alpha * (b - a)),  a = input_rgb[p][c],  b = pred_rgb[p][c]
 *                                     Image.blend(input, prediction, alpha), misc.py:342: the subtraction, the product
 *                                     and the sum each rounded to fp32, no FMA
 *     label_ids[p] = id_table[pred[p]]        the train-id -> label-id loop of misc.py:318-322 as one table
 *     prob_u8[p]   = u8(prob[p] * 255.0f)     misc.py:314, 377-378
 *     err_u8[p]    = (err[p] * 255) & 255     misc.py:377-378 on the 0/1 error mask
 * Outside [0, 256) the reference's float -> byte cast is undefined behaviour; HERE u8 SATURATES (v <= 0 -> 0,
 * v >= 255 -> 255) and NaN gives 0.
 * image fp32 [3][H][W] with plane stride plane_stride >= H*W elements; gts int64 [H][W]; pred, err uint8 [H][W]; prob
 * fp32 [H][W]; palette 256 x 3 bytes and id_table 256 bytes on the DEVICE; the *_rgb outputs uint8 [H][W][3], the
 * others uint8 [H][W].  Every input and output is optional; an output is written when it is given.  SSA_EINVAL (before
 * the device is touched) when no output is given, when an output lacks an input it is made from (input_rgb: image,
 * inv_mean3, inv_std3; gt_rgb: gts, palette; pred_rgb: pred, palette; comp_rgb: those of input_rgb and pred_rgb and
 * 0 <= alpha <= 1; label_ids: pred, id_table; prob_u8: prob; err_u8: err) and for H < 1 || W < 1.  Pointers on the grid
 * of their wide access (image, gts, prob 16 bytes with plane_stride % 4 == 0; everything else 4 bytes) take the wide
 * path, four pixels per thread and step; any other alignment is served pixel by pixel with the same result.       */
int ssa_dump_tail(const float* image, long plane_stride, const float* inv_mean3, const float* inv_std3,
                  const int64_t* gts, const unsigned char* pred, const unsigned char* palette,
                  const unsigned char* id_table, const float* prob, const unsigned char* err, float alpha,
                  int H, int W, unsigned char* input_rgb, unsigned char* gt_rgb, unsigned char* pred_rgb,
                  unsigned char* comp_rgb, unsigned char* label_ids, unsigned char* prob_u8, unsigned char* err_u8,
                  void* stream);

/* out[i] = u8(mask[i] * 255.0f) over n fp32 values, u8 as above (saturating, NaN -> 0): the attn_* assets of
 * ImageDumper.dump (misc.py:373-378), which live at sizes of their own.  SSA_EINVAL for a null pointer or n < 1.   */
int ssa_mask_u8(const float* mask, long n, unsigned char* out, void* stream);

/* Optimizer step (train.py:509 on the torch.optim.SGD of loss/optimizer.py:47-53;
 * SURVEY.md 8f rank 3): for every tensor i, elementwise in fp32
 *     d = g + weight_decay*p;  buf = momentum*buf + d;  p -= lr * (nesterov ? d + momentum*buf : buf)
 * (torch's SGD with dampening 0; a momentum buffer starting at zero reproduces its
 * first step).  params/grads/bufs/numel are HOST arrays of n_tensors entries holding
 * device pointers to dense fp32 tensors; bufs may be NULL (momentum 0) and so may
 * single entries of it.  Up to 96 tensors go into one launch (pointers travel as
 * kernel arguments, so a captured graph owns them).  lr_dev, when not NULL, is a
 * device float read at run time instead of `lr` -- a captured step then follows the
 * LR schedule without re-capture.
 * amp_state (optional): the loss-scaling record of fp16 training, 4 device floats {scale, found_inf, clean steps,
 * 1 / scale}: every gradient is multiplied by amp_state[3] on the way in, and when amp_state[1] != 0 (an inf / nan
 * was found by ssa_amp_check_grads) the call changes NOTHING -- apex.amp's skipped step (train.py:503-505).          */
int ssa_sgd_momentum_step(void* const* params, const void* const* grads, void* const* bufs,
                          const int64_t* numel, int n_tensors, float lr, const float* lr_dev,
                          float momentum, float weight_decay, int nesterov, const float* amp_state,
                          void* stream);
/* Dynamic loss scaling (apex.amp's LossScaler, the reference's --fp16 path: train.py:380-381,503-505), capturable:
 * ssa_amp_check_grads sets amp_state[1] = 1 if any element of the n_tensors dense fp32 gradient tensors (HOST arrays
 * of device pointers / element counts, as above) is inf or nan;  ssa_amp_update then closes the step:
 * found_inf: scale = max(scale * backoff, min_scale), clean steps = 0; else clean steps += 1 and, on reaching
 * growth_interval, scale = min(scale * growth, max_scale), clean steps = 0; found_inf = 0; amp_state[3] = 1 / scale. */
int ssa_amp_check_grads(const void* const* grads, const int64_t* numel, int n_tensors, float* amp_state,
                        void* stream);
int ssa_amp_update(float* amp_state, int growth_interval, float growth, float backoff, float min_scale,
                   float max_scale, void* stream);
/* The same update, additionally counting what apex LOGS ("Gradient overflow.  Skipping step", apex/amp/scaler.py):
 * counters[0] += 1 and counters[1] += 1 on a skipped step, counters[1] = 0 on a clean one -- skipped steps in total and in
 * a row (2 floats of device memory, or NULL).  A run whose gradients are genuinely nan pins the scale at min_scale and
 * skips every step: the host reads this record (semseg_amd.amp.LossScaler.state_dict / .health) to say so. */
int ssa_amp_update_counted(float* amp_state, float* counters, int growth_interval, float growth, float backoff,
                           float min_scale, float max_scale, void* stream);

/* Adam, AMSGrad and RAdam (train.py:509 `optim.step()` on the torch.optim.Adam of loss/optimizer.py:55-59, mode 0, with
 * `--amsgrad` mode 1, or on the RAdam of loss/optimizer.py:60-63 = loss/radam.py:29-107, mode 2), the siblings of
 * ssa_sgd_momentum_step: HOST arrays of n_tensors device pointers to dense fp32 tensors, up to 56 tensors per launch,
 * the pointers travel as kernel arguments.  Whatever depends on the step count lives in a 16-byte device record per
 * parameter (16-byte aligned; zero-initialised = no step taken yet):
 *     { int32 t;  int32 rectified;  float c1;  float c2; }
 * ssa_adam_advance, one thread per record of the list: t += 1, then in double precision, rounded once,
 *     mode 0 / 1:  c1 = 1 / (1 - beta1^t),  c2 = 1 / sqrt(1 - beta2^t),  rectified = 1
 *     mode 2:      N_max = 2 / (1 - beta2) - 1,  N_sma = N_max - 2 t beta2^t / (1 - beta2^t),  rectified = N_sma >= 5,
 *                  c1 = rectified ? sqrt((1 - beta2^t)(N_sma - 4)/(N_max - 4) (N_sma - 2)/N_sma N_max/(N_max - 2)) / (1 - beta1^t)
 *                                 : 1 / (1 - beta1^t)
 * ssa_adam_step, elementwise in fp32 with the record of each tensor (call ssa_adam_advance on the same list first):
 *     mode 0 / 1:  g += weight_decay p;  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;
 *                  [mode 1: vmax = max(vmax, v)]   p -= lr c1 * m / (sqrt(v | vmax) c2 + eps)
 *     mode 2:      v = beta2 v + (1 - beta2) g g;  m = beta1 m + (1 - beta1) g;  p += -weight_decay lr p;
 *                  p -= lr c1 * (rectified ? m / (sqrt(v) + eps) : m)
 * max_exp_avg_sq is read in mode 1 only (NULL otherwise).  lr_dev and amp_state as in ssa_sgd_momentum_step: the
 * gradients are multiplied by amp_state[3], and when amp_state[1] != 0 BOTH calls change nothing -- a skipped step
 * leaves t, m, v, vmax and p as they were.  SSA_EINVAL for a mode outside 0..2, betas outside [0, 1), negative eps
 * or weight decay, and null or (records) misaligned pointers.                                                       */
int ssa_adam_advance(void* const* recs, int n_tensors, int mode, double beta1, double beta2,
                     const float* amp_state, void* stream);
int ssa_adam_step(void* const* params, const void* const* grads, void* const* exp_avg,
                  void* const* exp_avg_sq, void* const* max_exp_avg_sq, const void* const* recs,
                  const int64_t* numel, int n_tensors, int mode, float lr, const float* lr_dev,
                  double beta1, double beta2, float eps, float weight_decay, const float* amp_state,
                  void* stream);

/* fp32 elementwise out = a (+ | * | /) b (op 0 | 1 | 2) and its backward (da, db optional): the
 * attention normalisation and the attention-weighted sum over scales of the attention-to-scale
 * heads, network/attnscale.py:153-166,330-352.                                   */
int ssa_ewise_f32(int op, const float* a, const float* b, float* out, long n, void* stream);
int ssa_ewise_bwd_f32(int op, const float* a, const float* b, const float* dout, float* da,
                      float* db, long n, void* stream);

/* axpy on fp32: y = alpha*x + (accumulate? y : 0) */
int ssa_axpy_f32(const float* x, float alpha, float* y, long n, int accumulate,
                 void* stream);

/* ---------------------------------------------------------------- probes ----
 * Hardware-layout probes used by tests/test_probe_gpu.py (MFMA fragment and
 * ds_read_b64_tr_b16 lane maps are verified on the device, not assumed).      */
int ssa_probe_mfma32(const void* a, const void* b, float* c, void* stream);
int ssa_probe_tr16(unsigned short* out, int mode, void* stream);
/* c[16][16] = a[16][32] * b[32][16] (b given transposed: [16 n][32 k]) through v_mfma_f32_16x16x32; out[64][2] =
 * (a, b) of every lane after v_permlane16_swap of a = lane, b = lane + 100.                                  */
int ssa_probe_mfma16(const void* a, const void* bt, float* c, void* stream);
int ssa_probe_swap16(unsigned* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMSEG_HIP_H */
