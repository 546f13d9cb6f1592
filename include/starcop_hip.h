/*
 * starcop_hip.h -- C ABI of libstarcop_hip.so (gfx950 / MI355X).
 *
 * The reference (spaceml-org/STARCOP) is pure Python on stock torch ops; it has
 * no FFI of its own.  Each entry point below therefore replaces the *torch op
 * sequence* the reference dispatches on its segmentation hot path, and cites the
 * reference lines whose arithmetic it implements.  A reference maintainer binds
 * these with ctypes; starcop_amd/_lib.py is that binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative sc_status; it never
 *     throws and never synchronises the device; the text of the last error on
 *     the calling thread is returned by sc_last_error().
 *   - all pointers are DEVICE pointers unless the parameter name ends in _host;
 *     tensors are dense NCHW fp32 unless stated; `stream` is a hipStream_t
 *     (pass torch.cuda.current_stream().cuda_stream).
 *   - no hidden allocation: scratch is caller-provided.
 */
#ifndef STARCOP_HIP_H
#define STARCOP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sc_stream;

enum sc_status {
  SC_OK = 0,
  SC_ERR_ARG = -1,      /* bad shape / unsupported configuration  -> ValueError        */
  SC_ERR_LAUNCH = -2,   /* HIP launch/runtime error               -> RuntimeError      */
  SC_ERR_NOTPD = -3,    /* covariance not positive definite       -> LinAlgError       */
  SC_ERR_NODEV = -4     /* no gfx950 device                       -> RuntimeError      */
};

/* how an activation tensor is read ("normalise on load") */
enum sc_src_mode {
  SC_SRC_RAW = 0,     /* v = x                                                              */
  SC_SRC_AFFINE = 1,  /* v = act(x*c[0] + c[1])            eval/train BatchNorm + ReLU/ReLU6 */
  SC_SRC_BNBWD = 2,   /* v = A*(pass(aux*c[0]+c[1]) ? x : 0) + B*aux + D,  (A,B,D)=c[2..4]  */
                      /*     x = dL/d(act(BN(y))), aux = y : BatchNorm+activation backward  */
  SC_SRC_NORM = 3     /* v = clamp((x-c[0])/c[1], c[2], c[3])   DataNormalizer.normalize_x  */
};
enum sc_act { SC_ACT_NONE = 0, SC_ACT_RELU = 1, SC_ACT_RELU6 = 2 };

#define SC_CST 8          /* floats of per-channel constants per channel            */
/* BatchNorm statistics are written as per-work-group partial rows [rows][C][2] (plain stores, no atomics,
 * deterministic) and summed in fp64 by sc_bn_finalize / sc_bn_bwd_finalize.  rows = sc_stat_rows(kind, ...) */
enum sc_stat_kind { SC_STAT_CONV3 = 0, SC_STAT_CONV1 = 1, SC_STAT_DW = 2, SC_STAT_STEM = 3, SC_STAT_BNBWD = 4,
                    SC_STAT_CONV1K = 5 /* sc_conv1x1_ksplit: one row per 32 pixels */,
                    SC_STAT_PW3 = 6 /* sc_conv1x1_pw3: one row per 32 flat pixels of the whole batch */ };

typedef struct sc_src {
  const float* x;    /* primary tensor  [N, C, H>>up, W>>up]                          */
  const float* aux;  /* secondary tensor (SC_SRC_BNBWD) or NULL                       */
  const float* cst;  /* per-channel constants [C][SC_CST] or NULL (SC_SRC_RAW)        */
  int32_t C;         /* channels of this source                                       */
  int32_t mode;      /* sc_src_mode                                                   */
  int32_t act;       /* sc_act                                                        */
  int32_t up;        /* 1: stored at half resolution, read with nearest x2 upsample   */
} sc_src;

/* ------------------------------------------------------------------------- */
/* library                                                                    */
const char* sc_last_error(void);
int sc_version(void);
int sc_device_check(void);   /* 0 iff the current device is gfx950 */

/* ------------------------------------------------------------------------- */
/* weights: pack OIHW -> kernel layouts (replaces nothing in the reference; it is
 * the layout step torch's conv backends do internally).
 *   fwd  : wpk[co_tile][ci][tap][co_in_tile]                (co_t = 16, 32 or 64; ci zero-padded to the K chunk)
 *   dgrad: same layout of the transposed+flipped filter: W'[ci][co][2-kh][2-kw]
 */
int sc_pack_weights(const float* w_oihw, float* wpk, int Cout, int Cin, int ks,
                    int co_t, int transpose_flip, sc_stream stream);
size_t sc_packed_weight_floats(int Cout, int Cin, int ks, int co_t, int transpose_flip);

/* every filter pack of a network in one launch.  `descs` and `block_starts` (n entries: first 256-thread block of each
 * descriptor, blocks = ceil(sc_pack_work_items / 256)) live in DEVICE memory and are built once by the caller;
 * bx3 = number of bf16 terms (3, 2 or 1) selects the sc_pack_weights_bx3 layout (ks must be 3); 0 = fp32 layout. */
typedef struct sc_pack_desc {
  const float* w; float* wpk;
  int32_t Cout, Cin, ks, co_t, transpose_flip, bx3;
  uint64_t total;        /* = sc_pack_work_items(...) */
} sc_pack_desc;
size_t sc_pack_work_items(int Cout, int Cin, int ks, int co_t, int transpose_flip, int bx3);
int sc_pack_weights_batch(const sc_pack_desc* descs_dev, const uint32_t* block_starts_dev, int n, uint32_t total_blocks,
                          sc_stream stream);

/* ------------------------------------------------------------------------- */
/* dense conv (groups=1, stride 1, pad ks/2, ks in {1,3}) as implicit GEMM on fp32 MFMA.
 * Replaces torch.nn.functional.conv2d (+ cat + interpolate(nearest) + batch_norm + relu/relu6
 * of the producers) as dispatched by smp.Unet at starcop/models/model_module.py:244,
 * and its backward-data when called with transpose_flip-packed weights.
 *   input  = channel concat of nsrc (1|2) sources, each with its own prologue
 *   output = out0 (channels [0,csplit)) and out1 (channels [csplit,Cout)); csplit==Cout -> single
 *            out = acc (+ add0) (+ add1) (+ old out if accum flag)
 *   stats  : if non-NULL, per-channel sum / sum-of-squares of acc over each work-group's pixel tile are written to
 *            stats[row][Cout][2] (float), row = n*tiles + tile, rows = sc_stat_rows(SC_STAT_CONV3|CONV1, N, H, W)
 * ks = 1 on planes of >= 8192 pixels (H*W % 256 == 0, 16-byte aligned tensors) with a short contraction (16-32 source channels, one plain
 * output of <= 160 channels, RAW / AFFINE or BNBWD source) runs on a streaming kernel (16-byte loads and stores, same fp32 products,
 * same statistics rows); everything else on the LDS-staged kernels.
 */
/* BatchNorm-backward sums of the tensor whose gradient a data-gradient launch writes into out0 (sc_conv3x3_bx3, sc_conv3x3_thin16,
 * sc_conv3x3_sp_dgrad): what sc_bn_bwd_reduce(out0, y, cst, act, ...) would compute by streaming both tensors again, left by the
 * launch that produces the gradient -- valid when that launch writes the COMPLETE gradient (single consumer: accum0 = 0, no add
 * tensors).  rows[sc_stat_rows(SC_STAT_CONV3, N, H, W)][C][2] (float) = {sum g', sum g' x_hat} over each work-group's pixel tile,
 * g' = out0 * act'(BN(y)), for sc_bn_bwd_finalize_rows32 (sc_conv3x3_sp_dgrad: not taken);
 * absmax (or NULL): raised (atomic max; zeroed by the caller) to max |scale_c g'|, the range hint of the SC_TERMS_F16X2 kernels. */
typedef struct sc_bnr_args {
  const float* y;        /* raw (pre-BatchNorm) values of the tensor, same shape as out0   */
  const float* cst;      /* its forward constants {scale, shift, mean, invstd, ..} [C][SC_CST] */
  int32_t act;           /* its activation (SC_ACT_*)                                       */
  float* rows;
  float* absmax;
} sc_bnr_args;
#define SC_TERMS_F16X2 4   /* `terms` code: two fp16 terms per operand with exact power-of-two range scaling (22 significand
                            * bits, three products: fp32-level accuracy at half the MFMA work of the three-term bf16 split) */
typedef struct sc_conv_args {
  sc_src src[2];
  int32_t nsrc;
  const float* wpk;      /* packed weights, see sc_pack_weights                 */
  int32_t N, H, W;       /* output (= input) spatial size                        */
  int32_t Cout;
  int32_t ks;            /* 1 or 3                                               */
  int32_t co_t;          /* 16 (thin layers, ks=3, Cout<=16), 32 or 64: cout tile the weights were packed for */
  float* out0; float* out1;
  int32_t csplit;        /* == Cout when there is a single output                */
  int32_t accum0, accum1;/* 1: out += result                                     */
  const float* add0;     /* optional [N,Cout,H,W] tensors added in the epilogue  */
  const float* add1;     /*   (only valid with csplit == Cout)                   */
  float* stats;          /* [rows][Cout][2] partial sums or NULL                 */
  int32_t terms;         /* sc_conv3x3_bx3 only: bf16 terms per operand, 0 or 3 = fp32-accurate split, 2 = two terms (2^-18), 1 = plain bf16 */
  int32_t down0;         /* sc_conv3x3_bx3 only: 1 = channels [0,csplit) are stored 2x2-summed at half resolution into out0
                          * ([N,csplit,H/2,W/2]): the backward of F.interpolate(scale_factor=2, mode="nearest") in
                          * smp's DecoderBlock fused into the data-gradient store (no full-resolution temporary) */
  const float* absmax;   /* terms == SC_TERMS_F16X2 with a BNBWD source: device float >= the tensor's max |A_c g| (written by
                          * sc_bn_bwd_reduce / sc_bn_bwd_small); NULL: the gradient operand is taken to be O(1)              */
  const float* xbound[2];/* terms == SC_TERMS_F16X2, forward sources: per source a device float >= max |activation| of that source
                          * (sc_bn_finalize(act_bound) in training, sc_add_srcs_absmax records) or NULL (ReLU6-bounded / unknown): the
                          * kernels scale the fp16 operand by 2 when 2 M <= 32752 and by the largest power of two with s M <= 32752
                          * otherwise, so a BatchNorm'd activation can never reach the +-65504 clamp                         */
  const sc_bnr_args* bnr;/* data-gradient launches (SC_SRC_BNBWD source): also leave the BatchNorm-backward sums of out0's tensor, or NULL */
} sc_conv_args;
int sc_conv2d_mfma(const sc_conv_args* a, sc_stream stream);
/* HOST: whether sc_conv2d_mfma hands these arguments (ks = 1) to its register-streaming pointwise kernel, and which variant of it:
 * -1 = no (the LDS-staged kernels take the launch), else 100 * (src[0] is SC_SRC_BNBWD) + 10 * NCB (16-channel output blocks per
 * wave: 1, 2, 5, 6 forward; 2, 3, 5, 6 for a BNBWD source) + NKS (K steps of 4 input channels in registers: 4, 6 or 8).  The pointers
 * are only tested for NULL and 16-byte alignment.  The entry point dispatches on this value. */
int sc_pw_stream_variant(const sc_conv_args* a);
/* 1x1 convolution for few-pixel / long-K layers (the <= 64^2 inverted-residual projections and the data gradients of the
 * expansions): 32-pixel tiles, the four waves of a work-group split K, operands go global -> registers -> MFMA (no LDS
 * staging).  Same arguments as sc_conv2d_mfma with ks = 1, nsrc = 1 and sc_pack_weights(ks=1) filters; co_t in {32, 64};
 * statistics rows = sc_stat_rows(SC_STAT_CONV1K, N, H, W). */
int sc_conv1x1_ksplit(const sc_conv_args* a, sc_stream stream);

/* The same 3x3 convolution (forward, or backward-data with transpose_flip-packed filters) with fp32 accuracy on the
 * bf16 matrix cores: every fp32 operand is split exactly into three bf16 terms while it is staged and the six partial
 * products of weight >= 2^-24 are accumulated in fp32 (6 x v_mfma_f32_32x32x16_bf16 per 32x32x16 block, 2.7x the
 * v_mfma_f32_32x32x2_f32 rate; error of the same order as one fp32 rounding per product).  Same arguments, prologues,
 * epilogue and statistics rows (SC_STAT_CONV3) as sc_conv2d_mfma with ks = 3; co_t in {32, 64}; `wpk` must come from
 * sc_pack_weights_bx3 (16-byte aligned).  A concat needs src[0].C % 16 == 0.
 * `terms` = 1 (args->terms and the pack call) keeps only the leading bf16 term of each operand: one MFMA per block, bf16
 * matrix math with fp32 accumulation -- the network's "bf16" precision mode (BASELINE configs[3]); tensors stay fp32.
 * `terms` = 2 keeps two terms per operand and the three products a0*b1 + a1*b0 + a0*b0 (operand error 2^-18): the opt-in
 * "fp32-bwd2" / "fp32-2" modes.
 * Replaces the same torch.nn.functional.conv2d calls as sc_conv2d_mfma (starcop/models/model_module.py:244). */
int sc_pack_weights_bx3(const float* w_oihw, float* wpk, int Cout, int Cin, int co_t, int transpose_flip, int terms,
                        sc_stream stream);
size_t sc_packed_weight_floats_bx3(int Cout, int Cin, int co_t, int transpose_flip, int terms);
int sc_conv3x3_bx3(const sc_conv_args* a, sc_stream stream);

/* weight gradient of the same conv: dW[co][ci][kh][kw] = sum_{n,y,x} dy * in.
 *   dy  : one source (normally SC_SRC_BNBWD: g + y of the conv output), Cout channels
 *   in  : concat of nsrc sources with the forward prologues, Cin channels
 *   part: scratch [nslices][taps][Cout_pad32][Cin_pad32]; call sc_wgrad_workspace_floats
 *   dw  : [Cout][Cin][ks][ks]  (overwritten)
 */
typedef struct sc_wgrad_args {
  sc_src dy;
  sc_src src[2];
  int32_t nsrc;
  int32_t N, H, W, Cout, Cin, ks;
  float* part; size_t part_floats;
  float* dw;
  int32_t terms;         /* sc_conv3x3_wgrad_bx3 only: 0 or 3 = fp32-accurate split, 2 = two terms, 1 = plain bf16 operands */
  const float* absmax;   /* terms == SC_TERMS_F16X2: scale hint of dy, as in sc_conv_args                                     */
  const float* xbound[2];/* terms == SC_TERMS_F16X2: activation bounds of the input sources, as in sc_conv_args               */
} sc_wgrad_args;
size_t sc_wgrad_workspace_floats(int N, int H, int W, int Cout, int Cin, int ks);
int sc_conv2d_wgrad_mfma(const sc_wgrad_args* a, sc_stream stream);
/* The same kernel without its trailing reduction launches: the K-slice partials stay in a->part (which must then be a buffer
 * of this layer's own, alive until the batch reduction) and `pending` (HOST struct) receives what sc_wgrad_reduce_batch needs.
 * A network's ~35 pointwise layers each end in 2-3 few-microsecond dependent launches otherwise; the batch sums all of them in
 * ONE launch at the end of the backward pass.  descs_dev / block_starts_dev: DEVICE arrays built once by the caller (the
 * descriptors do not change between steps), block_starts[i] = first 256-thread block of descriptor i, blocks_i = ceil(total_i/256). */
typedef struct sc_wgrad_pending {
  const float* part; float* dw;
  int32_t nparts, taps, Cout, Cin, CoP, CiP;
  uint64_t total;        /* taps * Cout * Cin */
} sc_wgrad_pending;
int sc_conv2d_wgrad_mfma_deferred(const sc_wgrad_args* a, sc_wgrad_pending* pending_host, sc_stream stream);
int sc_wgrad_reduce_batch(const sc_wgrad_pending* descs_dev, const uint32_t* block_starts_dev, int n, uint32_t total_blocks,
                          sc_stream stream);
/* Thin 3x3 layers (Cout <= 16, Cin = 16 or 32: smp's decoder.blocks.4 at full resolution) with two fp16 terms on
 * v_mfma_f32_16x16x32_f16: the filter bank stays in registers, all input channels are staged in one pass.  Same arguments as
 * sc_conv3x3_bx3 with terms = SC_TERMS_F16X2, nsrc = 1, a single plain output (csplit = Cout, no add / accumulate / down0);
 * `wpk` from sc_pack_weights_thin16 (or a sc_pack_desc with bx3 = SC_PACK_THIN16); statistics rows SC_STAT_CONV3.
 * Forward, or backward-data with transpose_flip-packed filters (then "Cout" is the layer's input channel count).
 * A 32-channel source with up = 1 (decoder.blocks.4.conv1: conv3x3 of a nearest-2x up-sampled tensor) runs as four 2x2 convolutions on
 * the half-resolution source (sub-pixel form: the pack of a forward filter with Cin = 32 carries the 16 phase filters behind its 3x3
 * entries).  down0 = 1 (the one exception to "no down0"): the data gradient of that layer -- 16-channel SC_SRC_BNBWD source at H x W,
 * Cout = csplit = 32 rows stored 2x2-summed into out0 [N,32,H/2,W/2] (accum0 allowed) -- from sc_pack_weights_thin16(Cout = 16,
 * Cin = 32, transpose_flip = 1), which packs the 4 x 4-position gathered filters of that form (no statistics / bnr / add epilogue). */
#define SC_PACK_THIN16 5
#define SC_PACK_PW3 6      /* sc_pack_desc.bx3 code of the pointwise layout of sc_conv1x1_pw3 (ks = 1; co_t ignored) */
size_t sc_packed_weight_floats_thin16(int Cout, int Cin, int transpose_flip);
int sc_pack_weights_thin16(const float* w_oihw, float* wpk, int Cout, int Cin, int transpose_flip, sc_stream stream);
int sc_conv3x3_thin16(const sc_conv_args* a, sc_stream stream);

/* Decoder conv1 as a SUB-PIXEL convolution: smp's DecoderBlock runs conv3x3(cat([interpolate(prev, x2, "nearest"), skip]))
 * (starcop/models/model_module.py:244-251).  For the up-sampled channels, conv3x3(nearest_up2(x)) is exactly four phase-specific
 * 2x2 convolutions on the LOW-resolution x (phase filter = sum of the taps that land on the same source pixel; zero padding maps
 * 1:1): 2.25x fewer multiply-adds and every low-resolution value staged once instead of once per high-resolution copy.  The
 * skip channels join the same launch as four low-resolution "parity planes" each (csrc/conv_sp_pack.h).
 *   sc_conv3x3_sp: sc_conv_args with src[0] = the half-resolution tensor (up = 1), optional src[1] = the full-resolution skip
 *   tensor (up = 0), both RAW or AFFINE; H x W = OUTPUT size (even); ks = 3; terms = SC_TERMS_F16X2 (the two-fp16-term arithmetic
 *   of sc_conv3x3_bx3) or 1 (one bf16 term per operand: the "bf16" precision mode; xbound unused); csplit = Cout, one plain output (no add / accumulate / down0); co_t ignored (32); `wpk` from
 *   sc_pack_weights_sp (or a sc_pack_desc with bx3 = SC_PACK_SP, Cin = the filter's total input channels and co_t = how many
 *   of them, the leading ones, belong to the up-sampled source; transpose_flip = 4 for the one-bf16-term layout); statistics rows = sc_sp_stat_rows(N, H, W, Cout) (one per work-group tile: 8 x 32 low-resolution pixels; 16 x 16 -- or, for launches of at most 128 such work-groups, 8 x 16 -- on planes narrower than 32). */
#define SC_PACK_SP 7
size_t sc_packed_weight_floats_sp(int Cout, int Cup, int Cskip);
int sc_pack_weights_sp(const float* w_oihw, float* wpk, int Cout, int Cup, int Cskip, int terms, sc_stream stream);
int sc_sp_stat_rows(int N, int H, int W, int Cout);
int sc_conv3x3_sp(const sc_conv_args* a, sc_stream stream);
/* ... and its data gradient w.r.t. the half-resolution source: a stride-2 4x4 convolution of dy (four parity planes x 2x2 taps), written
 * at half resolution directly -- no full-resolution gradient of the up-sampled channels, no 2x2 down-sum (replaces
 * sc_conv3x3_bx3(down0 = 1) on those channels; the skip channels' gradient stays an ordinary 3x3 launch).
 *   sc_conv3x3_sp_dgrad: sc_conv_args with nsrc = 1, src[0] = the SC_SRC_BNBWD operand of the layer's output (g, y, constants; H x W),
 *   Cout = csplit = the up-sampled source's channels, out0 = [N, Cout, H/2, W/2] (accum0 allowed), terms = SC_TERMS_F16X2 or 1, absmax as
 *   in sc_conv3x3_bx3; `wpk` from sc_pack_weights_spd (or a sc_pack_desc with bx3 = SC_PACK_SPD, Cin = the filter's total input
 *   channels, co_t = the up-sampled source's channels, transpose_flip = 2 for vskip, | 4 for the one-bf16-term layout).
 *   vskip (sc_spd_vskip_ok: <= 64 up-sampled and <= 16 skip channels, smp's decoder.blocks.3): the skip channels' full-resolution
 *   gradient rides along in the otherwise idle half of the 128-channel tile -- Cout = all input channels, csplit = the up-sampled ones,
 *   out1 = [N, Cout - csplit, H, W] (accum1 allowed): ONE launch stages dy for both gradients.
 *   skip tiles (any other channel counts, out1 given; pack with vskip = 2 / transpose_flip = 3): the skip channels' gradient as
 *   additional 128-channel tiles of the launch (32 skip channels x 4 output parities each) -- same arguments as vskip; which of the two
 *   forms a launch takes follows from sc_spd_vskip_ok(csplit, Cout - csplit), so the pack must be made with the matching mode. */
#define SC_PACK_SPD 8
size_t sc_packed_weight_floats_spd(int Cout, int Cup, int Cskip_tiles /* skip channels packed as skip tiles (vskip = 2), else 0 */);
int sc_spd_vskip_ok(int Cup, int Cskip);
int sc_pack_weights_spd(const float* w_oihw, float* wpk, int Cout, int CinTotal, int Cup, int vskip, int terms, sc_stream stream);
int sc_conv3x3_sp_dgrad(const sc_conv_args* a, sc_stream stream);
/* ... and the weight gradient of its up-sampled channels as a PLAIN GEMM: up(x) is constant over 2x2 blocks of the output grid, so
 * dW[co][ci][kh][kw] = sum_q x[ci][q] * S_(kh,kw)[co][q] with S the tap-aligned 2x2 box sums of dy -- nine GEMMs over the low-resolution
 * pixels with no spatial shift, a quarter of the 3x3 form's multiply-adds (csrc/conv_spw.hip: box sums + exact two-fp16-term split in
 * one pass over (g, y); the activated, split source; a two-term fp16 GEMM; a fixed-order reduction of its K slices).
 *   sc_conv3x3_sp_wgrad: sc_wgrad_args with nsrc = 1, src[0] = the half-resolution tensor (up = 1; RAW / AFFINE; xbound[0]), dy = the
 *   layer's output gradient (H x W, even; normally SC_SRC_BNBWD; absmax), Cin = the FILTER's total input channels, terms =
 *   SC_TERMS_F16X2; writes dw[co][ci][3][3] for ci < src[0].C inside the [Cout][Cin][3][3] gradient (part / part_floats unused);
 *   `ws`: sc_sp_wgrad_workspace_bytes(N, H, W, Cout, src[0].C) bytes, 256-byte aligned.
 *   sc_wgrad_scatter_cols: a dense [Cout][Ccols][3][3] gradient (the skip channels', from sc_conv3x3_wgrad_bx3 on the skip source
 *   alone) into columns [col_off, col_off + Ccols) of the [Cout][CinTotal][3][3] gradient. */
size_t sc_sp_wgrad_workspace_bytes(int N, int H, int W, int Cout, int Cup);
int sc_conv3x3_sp_wgrad(const sc_wgrad_args* a, void* ws, size_t ws_bytes, sc_stream stream);
int sc_wgrad_scatter_cols(const float* src, float* dw, int Cout, int Ccols, int CinTotal, int col_off, sc_stream stream);
/* HOST queries (no GPU work): which kernel instantiation the three sub-pixel entry points launch for these arguments, with
 * STARCOP_SP_NPP applied; -1 for arguments the entry point rejects (the reason is left in sc_last_error).  Pointers are only tested
 * for NULL and alignment; the workspace of the weight gradient is not looked at.  The entry points dispatch on these values.
 *   sc_sp_variant (sc_conv3x3_sp):  100 * (TW / 16) + 10 * NPP + M for k_conv3_sp<TW, M == 1, NPP> -- TW = 32 from 32 low-resolution
 *     columns, else 16; NPP = 2 (256-pixel tiles) when N x the 256-pixel tiles x the 32-channel output tiles exceed 128 work-groups,
 *     else 1 (sc_sp_stat_rows counts the tiles of the same NPP); M = 4: two fp16 terms, 1: one bf16 term.  8 codes.
 *   sc_spd_variant (sc_conv3x3_sp_dgrad):  1000 * skip_mode + the same code for k_conv3_spd<TW, M == 1, NPP>, its channel tiles being
 *     ntu + nts (128 up-sampled channels each + in mode 2 32 skip channels each); skip_mode 0: no out1, 1: virtual skip channels
 *     (sc_spd_vskip_ok), 2: skip tiles -- a run-time branch with its own store path and pack layout.  24 codes.
 *   sc_sp_wgrad_variant (sc_conv3x3_sp_wgrad):  CB of k_spw_gemm<CB>: 2 above 64 up-sampled channels, else 1. */
int sc_sp_variant(const sc_conv_args* a);
int sc_spd_variant(const sc_conv_args* a);
int sc_sp_wgrad_variant(const sc_wgrad_args* a);

/* weight gradient of the same thin layers (Cout <= 16, Cin = 16 | 32, one source which may be upsampled) with two fp16 terms on
 * v_mfma_f32_16x16x32_f16: same sc_wgrad_args as sc_conv2d_wgrad_mfma with terms = SC_TERMS_F16X2 (absmax = the dy range hint),
 * workspace from sc_wgrad_thin16_workspace_floats.  Replaces the fp32-MFMA thin weight gradient (the step's last MFMA-bound fp32 kernel). */
size_t sc_wgrad_thin16_workspace_floats(int N, int H, int W, int Cout, int Cin);
int sc_conv3x3_wgrad_thin16(const sc_wgrad_args* a, sc_stream stream);

/* Pointwise (1x1) convolutions on the 16-bit matrix cores with fp32 accuracy (every fp32 operand split exactly into three bf16
 * terms, six products, fp32 accumulation: the arithmetic of sc_conv3x3_bx3 with terms = 3), without LDS staging: the MobileNetV2
 * encoder's expansion / projection convolutions (torchvision InvertedResidual.conv, smp.Unet's encoder at
 * starcop/models/model_module.py:244-251), forward or backward-data (transpose_flip-packed filters, SC_SRC_BNBWD source).
 * Same sc_conv_args as sc_conv2d_mfma with ks = 1, nsrc = 1, a single output (csplit = Cout; add0 / accum0 allowed; no add1,
 * out1, down0, bnb_*); `wpk` from a sc_pack_desc with bx3 = SC_PACK_PW3 (sc_packed_weight_floats_pw3 floats); co_t / terms are
 * ignored; statistics rows = sc_stat_rows(SC_STAT_PW3, N, H, W) = one row per 32 flat pixels of the batch. */
size_t sc_packed_weight_floats_pw3(int Cout, int Cin, int transpose_flip);
int sc_conv1x1_pw3(const sc_conv_args* a, sc_stream stream);
/* HOST: the kernel variant sc_conv1x1_pw3 launches for this shape (Cout = the launch's output channels: the layer's Cin for a data
 * gradient) -- the 32-channel output blocks a wave owns: 4, 2 or 1; -1 for a bad shape.  The entry point dispatches on this value. */
int sc_conv1x1_pw3_variant(int N, int H, int W, int Cout);
/* its weight gradient (K = pixels; H*W must be a multiple of 8): same sc_wgrad_args as sc_conv2d_wgrad_mfma with ks = 1, nsrc = 1;
 * workspace from sc_wgrad_pw3_workspace_floats; pending != NULL defers the sum over the K-slice partials to
 * sc_wgrad_reduce_batch (as sc_conv2d_wgrad_mfma_deferred), NULL finishes it here. */
size_t sc_wgrad_pw3_workspace_floats(int N, int H, int W, int Cout, int Cin);
int sc_conv1x1_wgrad_pw3(const sc_wgrad_args* a, sc_wgrad_pending* pending_host, sc_stream stream);
/* HOST: the kernel variant sc_conv1x1_wgrad_pw3 launches: 10 * tm + tn, the 32-channel blocks of dy (tm) and of the input (tn) a
 * wave owns -- 11, 12, 21 or 22; -1 for a bad shape.  The entry point dispatches on this value. */
int sc_wgrad_pw3_variant(int N, int H, int W, int Cout, int Cin);

/* One launch per MobileNetV2 inverted-residual block in INFERENCE (conv_irb.hip; torchvision InvertedResidual.conv inside
 * smp.Unet('mobilenet_v2').encoder, eval-mode BatchNorm: starcop/models/model_module.py:90-98 forward, :244-251 the network; the
 * notebook / padded_predict path starcop/models/utils/padding.py:13-50):
 *     x -> conv1x1 (Cin -> hidden) -> BN_e + ReLU6 -> depthwise 3x3 (stride 1 | 2, pad 1) -> BN_d + ReLU6 -> conv1x1 (hidden -> Cout)
 *       -> raw p (residual = 0: BN_p is the consumers' business, as for every other convolution here)
 *       -> z = x + BN_p(p)  (residual = 1: Cin == Cout; x as the source forms it, an AFFINE source's scale, shift and activation
 *          applied; z_absmax, if not NULL, is raised to max |z| like sc_add_srcs_absmax does)
 * The expanded tensors never leave the CU.  Both 1x1 filters come in the sc_conv1x1_pw3 layout (sc_pack_weights_batch with
 * SC_PACK_PW3, transpose_flip 0); fp32 accuracy (three exact bf16 terms per operand, six MFMA products, fp32 stencil).
 * Stride 1: 8 <= Cin <= 160, hidden % 32 == 0, Cout <= 384 subject to the accumulator budget; stride 2 (no residual; H, W are the INPUT
 * plane, the output is ((H - 1) / 2 + 1) x ((W - 1) / 2 + 1)): Cin <= 96, hidden % 64 == 0 (sc_irb_supported).  gfx950 only: the kernel
 * needs its 160 KB of LDS per work-group (the stride-2 tiling and every block with Cin > 96 use more than 64 KB). */
typedef struct sc_irb_args {
  sc_src x;                  /* block input [N,Cin,H,W]: SC_SRC_RAW or SC_SRC_AFFINE                                  */
  const float* wpk_expand;   /* PW3 pack of the expansion filter [hidden][Cin]                                         */
  const float* cst_expand;   /* [hidden][SC_CST]: {scale, shift, ..} of BN_e (sc_bn_finalize, eval)                    */
  const float* w_dw;         /* [hidden][3][3]                                                                         */
  const float* cst_dw;       /* [hidden][SC_CST] of BN_d                                                               */
  const float* wpk_project;  /* PW3 pack of the projection filter [Cout][hidden]                                       */
  const float* cst_project;  /* [Cout][SC_CST] of BN_p (residual = 1) or NULL                                          */
  float* out;                /* [N,Cout,Ho,Wo]: raw p, or z                                                            */
  float* z_absmax;           /* device float raised to max |z| (residual = 1) or NULL                                  */
  int32_t N, Cin, hidden, Cout, H, W, stride, residual;
} sc_irb_args;
int sc_irb_supported(int Cin, int hidden, int Cout, int H, int W, int stride);
/* HOST: the kernel variant sc_irb_eval launches for a block shape: -1 = unsupported, else
 *   10000 * tiling (0 = A: 4 x 8 output pixels, 64-channel chunks; 1 = B: 8 x 8, 32-channel chunks; 3 = the stride-2 form of A;
 *   2 was a third tiling that lost to A and is gone) + 1000 * projection pairs per wave (1..3)
 *   + 10 * expansion K steps held in registers (2, 4, 6 or 10) + work-groups per CU (1 | 2).
 * The entry point dispatches on this value. */
int sc_irb_variant(int Cin, int hidden, int Cout, int stride);
int sc_irb_eval(const sc_irb_args* a, sc_stream stream);

/* Fused TRAINING execution of the expansion + depthwise pair of a STRIDE-2 MobileNetV2 inverted-residual block (torchvision
 * InvertedResidual.conv[0..1] inside smp.Unet('mobilenet_v2'): starcop/models/model_module.py:244-251; train-mode BatchNorm):
 *     e = conv1x1(x, w_expand) -> BN_e + ReLU6 -> depthwise 3x3 (stride 2, pad 1) -> d (raw; BN_d is the consumers' business)
 * The 6x-expanded tensor e (four times the size of d) and its gradient are NEVER stored: every sweep recomputes e from the block
 * input x on the matrix cores (fp32 accuracy: three exact bf16 terms per operand, six products).  Replaces, per block and step,
 *   sc_conv1x1_* (expand, +stats) | sc_dwconv3x3_fwd | sc_dwconv3x3_bwd_fused | expand data gradient | expand weight gradient.
 * Cin in {8, 16, 24, 32}, hidden <= 192, H % 4 == 0, W % 8 == 0, stride 2 (sc_irt_supported).
 *   forward :  sc_irt_expand_stats -> sc_bn_finalize(BN_e, rows = sc_irt_rows(0,..)) -> sc_irt_fwd -> sc_bn_finalize(BN_d, rows =
 *              sc_irt_rows(1,..)) -> the projection convolution reads d as an SC_SRC_AFFINE source, as before
 *   backward:  (dy_d = the SC_SRC_BNBWD source of d, from sc_bn_bwd_* on d;  `work`: sc_irt_bwd_workspace_floats floats, 16-byte aligned)
 *              sc_irt_bwd        ONE sweep over (dy_d, x): e_sums rows for sc_bn_bwd_finalize(BN_e) (rows = sc_irt_bwd_rows), the
 *                                depthwise filter gradient (dw_acc[hidden][9] +=, fp64 atomics, as sc_dwconv3x3_bwd_fused), partial
 *                                rows of G = sum_px g'_e x^T and the part of dx that does not depend on the batch sums,
 *                                W_e^T (scale (.) g'_e), into `work`
 *              sc_bn_bwd_finalize(BN_e) -> cst_bwd_expand (.., .., A, B, D)
 *              sc_irt_bwd_fix    dx = that part + Q x + r (+ add0) (+ dx),  Q = W_e^T diag(B) W_e, r = W_e^T D: exact, because
 *                                dy_e = A g'_e + B e + D is affine per channel and e = W_e x
 *              sc_irt_xmoments   M = sum_px x x^T, s = sum_px x into `work` (any time after x exists; off the critical path)
 *              sc_irt_wgrad_finalize  dw_expand[hidden][Cin] = A (.) G + B (.) (W_e M) + D (x) s                              */
typedef struct sc_irt_args {
  sc_src x;                 /* block input [N,Cin,H,W]: SC_SRC_RAW or SC_SRC_AFFINE                                   */
  const float* w_expand;    /* [hidden][Cin]   (the 1x1 filter, OIHW)                                                 */
  const float* w_dw;        /* [hidden][3][3]                                                                         */
  const float* cst_expand;  /* [hidden][SC_CST] forward constants of BN_e (sc_bn_finalize); unused by sc_irt_expand_stats */
  int32_t N, Cin, hidden, H, W, stride;
} sc_irt_args;
int sc_irt_supported(int Cin, int hidden, int H, int W, int stride);
int sc_irt_rows(int stage, int N, int H, int W, int stride);        /* stage 0: sc_irt_expand_stats, 1: sc_irt_fwd */
int sc_irt_bwd_rows(int N, int hidden, int H, int W);
size_t sc_irt_bwd_workspace_floats(int N, int Cin, int hidden, int H, int W);
/* HOST only (no GPU touched): the launch geometry of the sweeps above for a block, as the launchers themselves derive it (they read
 * the same function).  SC_ERR_ARG for a block sc_irt_supported rejects, N <= 0 or N H W hidden >= 2^31.  out[SC_IRT_GEO_FIELDS]:
 *   [0] NKS          K steps of 16 input channels (template argument of the kernels)
 *   [1] nch          chunks of 32 hidden channels            [2] ngroups     chunk groups of <= 3 chunks = grid.y of k_irt_bwd
 *   [3] stats grid   work-groups of k_irt_stats (<= 512)     [4] pixel blocks  flat 32-pixel blocks of N H W (4 per work-group and trip)
 *   [5] fwd tiles    tiles of 4 x 16 outputs                 [6] fwd per_cu  work-groups per CU at the kernel's LDS size (1..4)
 *   [7] fwd grid     min(tiles, 256 per_cu) persistent work-groups of k_irt_fwd
 *   [8] bwd tiles    tiles of 4 x 32 e pixels                [9] tiles_per_wg  consecutive tiles one k_irt_bwd work-group walks
 *   [10] bwd rows    grid.x of k_irt_bwd = sc_irt_bwd_rows   [11] moments grid  work-groups of k_irt_xmom (<= 256)
 *   [12] moments K steps  16-pixel steps per k_irt_xmom work-group (4 waves x 4 steps per trip)
 *   [13] fix grid    work-groups of k_irt_fix (<= 1024) over the pixel blocks of [4]                                            */
#define SC_IRT_GEO_FIELDS 14
int sc_irt_geometry(int N, int Cin, int hidden, int H, int W, int stride, int* out);
int sc_irt_expand_stats(const sc_irt_args* a, float* stats /*[rows][hidden][2]*/, sc_stream stream);
int sc_irt_fwd(const sc_irt_args* a, float* d_out /*[N,hidden,Ho,Wo] raw*/, float* stats_d /*[rows][hidden][2] or NULL (inference)*/, sc_stream stream);
int sc_irt_bwd(const sc_irt_args* a, const sc_src* dy_d, double* e_sums /*[rows][hidden][2]*/, double* dw_acc /*[hidden][9]*/,
               float* work, sc_stream stream);
int sc_irt_xmoments(const sc_irt_args* a, float* work, sc_stream stream);
int sc_irt_bwd_fix(const sc_irt_args* a, const float* cst_bwd_expand, float* work, float* dx, const float* add0, int accum,
                   sc_stream stream);
int sc_irt_wgrad_finalize(const sc_irt_args* a, const float* cst_bwd_expand, float* work, float* dw_expand, sc_stream stream);

/* the 3x3 weight gradient with split-bf16 operands on the bf16 matrix cores (see sc_conv3x3_bx3); same arguments,
 * ks must be 3; workspace from sc_wgrad_bx3_workspace_floats */
size_t sc_wgrad_bx3_workspace_floats(int N, int H, int W, int Cout, int Cin);
int sc_conv3x3_wgrad_bx3(const sc_wgrad_args* a, sc_stream stream);

/* HOST queries (no GPU work): which kernel instantiation the four 3x3 matrix-core entry points of conv_bx3.hip launch for these
 * arguments, with the development knobs of the environment applied; -1 for arguments the entry point rejects (the reason is left in
 * sc_last_error).  Pointers are only tested for NULL and alignment; the workspace size of the weight gradients is not looked at.
 * The entry points dispatch on these values.  M = 1, 2, 3: that many bf16 terms per operand (terms 0 = 3), 4: two fp16 terms.
 *   sc_conv3_variant (sc_conv3x3_bx3):  1000 * WS + 100 * Q + 10 * BNB + M -- WS: the wave-specialised k_conv3_ws<Q, BNB> (M = 4 only),
 *     else k_conv3_bx3<Q, BNB, ..>; Q = co_t / 32; BNB: src[0] is SC_SRC_BNBWD
 *   sc_thin16_variant (sc_conv3x3_thin16):  100 * (C / 16) + 10 * BNB for k_conv3_thin_h<C, BNB> (100, 110, 200, 210),
 *     1200 = k_conv3_thin_sp (every up-sampled 32-channel RAW / AFFINE source; 200: not up-sampled), 2110 = k_conv3_thin_spd (down0)
 *   sc_wgrad3_variant (sc_conv3x3_wgrad_bx3):  10000 * PIPE + 1000 * M + 100 * WM + 10 * NCI + R for k_wgrad3_bx3<WM, .., NCI, .., PIPE>;
 *     R = 1: the kernel sums its K parts itself (sc_wgrad_finish sees one row per slice)
 *   sc_wgrad_thin16_variant (sc_conv3x3_wgrad_thin16):  100 * (Cin / 16) + 10 * (dy is SC_SRC_BNBWD) for k_wgrad_thin_h<Cin, BNB> */
int sc_conv3_variant(const sc_conv_args* a);
int sc_thin16_variant(const sc_conv_args* a);
int sc_wgrad3_variant(const sc_wgrad_args* a);
int sc_wgrad_thin16_variant(const sc_wgrad_args* a);

/* ------------------------------------------------------------------------- */
/* depthwise 3x3 (groups=C, pad 1, stride 1|2): forward, backward-data, backward-weight */
int sc_dwconv3x3_fwd(const sc_src* in, const float* w /*[C][3][3]*/, float* out,
                     int N, int C, int Hin, int Win, int stride, float* stats /* rows: SC_STAT_DW on (Hout,Wout) */,
                     sc_stream stream);
/* Producer-tail BatchNorm finalize: the launch that writes a tensor's statistics rows also finalizes that tensor's BatchNorm (what
 * sc_bn_finalize(stats, rows, count, ..) does in a launch of its own, ~5 us of idle chip behind every producer of the training
 * forward).  The work-group that arrives LAST for a channel -- a ticket per channel: `tickets[C]`, zero-initialised ONCE, counts
 * monotonically over launches -- sums that channel's rows in a fixed order (fp64) and writes constants, running statistics and the
 * activation bound: bit-reproducible whichever work-group does it. */
typedef struct sc_bn_tail {
  const float* gamma; const float* beta;      /* BatchNorm weight / bias [C]                              */
  float* running_mean; float* running_var;    /* updated with `momentum` (training semantics)              */
  float momentum, eps;
  float* cst;                                 /* [C][SC_CST] forward constants {scale, shift, mean, invstd} */
  float* act_bound;                           /* as in sc_bn_finalize, or NULL                             */
  uint32_t* tickets;                          /* [C]                                                       */
} sc_bn_tail;
/* sc_dwconv3x3_fwd + the BatchNorm of its output finalized by the launch itself (the depthwise layers of a batch leave 16-32 rows
 * per channel: the last (image, tile) of a channel reads 128-256 bytes) */
int sc_dwconv3x3_fwd_bn(const sc_src* in, const float* w, float* out, int N, int C, int Hin, int Win, int stride, float* stats,
                        const sc_bn_tail* bn, sc_stream stream);
int sc_dwconv3x3_dgrad(const sc_src* dy, const float* w, float* dx, int accum,
                       int N, int C, int Hin, int Win, int stride, sc_stream stream);
int sc_dwconv3x3_wgrad(const sc_src* dy, const sc_src* in, double* dw_acc /*[C][9] zeroed*/,
                       int N, int C, int Hin, int Win, int stride, sc_stream stream);
/* the three of them in one pass: dx (overwritten), dw_acc (+=, fp64 atomics) and, if in_sums != NULL, the BatchNorm-backward
 * partial sums of the INPUT tensor, in_sums[row][C][2] = {sum g_bn, sum g_bn * xhat}, g_bn = dx * act'(BN(y_in)), rows =
 * sc_stat_rows(SC_STAT_DW, N, Hin, Win) -- what sc_bn_bwd_reduce(dx, y_in) would compute by streaming both tensors again
 * (`in` must then be the SC_SRC_AFFINE source of that BatchNorm'd tensor with its cst_fwd constants).  In a MobileNetV2
 * inverted-residual block both sides of the depthwise conv are the 6x-expanded tensors: this kernel reads (g, y) of the
 * output once instead of twice and saves the (dx, y_in) pass of the expansion's BatchNorm backward. */
int sc_dwconv3x3_bwd_fused(const sc_src* dy, const sc_src* in, const float* w, float* dx, double* dw_acc, double* in_sums,
                           int N, int C, int Hin, int Win, int stride, sc_stream stream);
/* HOST: the kernel variant a depthwise entry point launches for a shape.  op: 0 = sc_dwconv3x3_fwd / _fwd_bn, 1 = _dgrad, 2 = _wgrad,
 * 3 = _bwd_fused; aligned16: whether every tensor pointer the entry point tests for 16-byte alignment passes (in->x and out for 0;
 * dy->x, dy->aux, in->x and dx for 3; ignored for 1 and 2).  -1 = the entry point rejects the arguments (stride outside {1, 2}; odd
 * sizes at stride 2 for op 3), 9016 = the wave-per-plane kernel (16 x 16 planes at stride 1, N C % 4 == 0),
 * else 1000 * stride + 10 * TW + V4: TW = tile width 64 | 32 | 16 (64 x 32, 32 x 32, 16 x 16 pixels per work-group, by the width of
 * the plane the work-groups tile: the output for ops 0 and 2, the input for 1 and 3), V4 = 1 for float4 staging, 0 for element-wise
 * staging (always 0 for ops 1 and 2).  The entry points dispatch on this value. */
int sc_dw_variant(int op, int N, int C, int Hin, int Win, int stride, int aligned16);
int sc_cast_f64_f32(const double* in, float* out, size_t n, sc_stream stream);
/* the same for n_descs (in, out, n) triples in one launch; descs_dev: DEVICE array (static for a plan: the caller builds it once).
 * The depthwise filter gradients of a backward walk (fp64 accumulators of sc_dwconv3x3_bwd_fused -> the flat fp32 gradient). */
typedef struct sc_cast_desc { const double* in; float* out; uint64_t n; } sc_cast_desc;
int sc_cast_f64_f32_batch(const sc_cast_desc* descs_dev, int n_descs, sc_stream stream);

/* stem: conv 3x3 stride 2 pad 1, Cin<=16 -> 32, input read through its prologue
 * (SC_SRC_NORM fuses DataNormalizer.normalize_x, starcop/data/normalizer_module.py:134-135).  Cin <= 8: the HyperSTARCOP inputs
 * (models/model_module.py:244-251), with or without statistics rows; 9 <= Cin <= 16: the 13 Sentinel-2 bands of the cloud detector
 * (starcop/sentinel2/models.py:63-78), inference only -- stats must be NULL.  sc_stem_conv_wgrad keeps Cin <= 8. */
int sc_stem_conv_fwd(const sc_src* in, const float* w /*[32][Cin][3][3]*/, float* out,
                     int N, int Cin, int Hin, int Win, float* stats /* rows: SC_STAT_STEM on (Hout,Wout) */,
                     sc_stream stream);
/* the kernel sc_stem_conv_fwd launches for (Cin, input width, 16-byte alignment of out); SC_ERR_ARG for Cin outside [1,16] */
enum sc_stem_kernel { SC_STEM_K_MFMA4 = 0, SC_STEM_K_VALU4 = 1, SC_STEM_K_VALU8 = 2, SC_STEM_K_VALU16 = 3 };
int sc_stem_fwd_kernel(int Cin, int Win, int out_aligned16);
/* HOST: the instantiation sc_stem_conv_wgrad launches, k_stem_wgrad<NJB>: NJB = the 16-column blocks of the (ci, tap) axis a wave
 * carries -- 3 for Cin <= 5 (9 Cin <= 48), 5 for Cin 6..8; SC_ERR_ARG for Cin outside [1,8].  The entry point dispatches on this value. */
int sc_stem_wgrad_njb(int Cin);
/* HOST: the work-groups of that launch = the partial rows [32][Cin][9] it leaves: min(N x tiles of 4 x 32 output pixels, 1024); with
 * more tiles than that a work-group walks several (tile += rows).  The rows are summed 16 at a time: no intermediate level up to 16
 * rows, one up to 256, two above.  SC_ERR_ARG for a non-positive size. */
int sc_stem_wgrad_rows(int N, int Hin, int Win);
size_t sc_stem_wgrad_workspace_floats(int N, int Cin, int Hin, int Win);
int sc_stem_conv_wgrad(const sc_src* dy, const sc_src* in, float* part, size_t part_floats,
                       float* dw, int N, int Cin, int Hin, int Win, sc_stream stream);

/* segmentation head: conv 3x3 pad 1, Cin -> 1, bias (fwd/dgrad/wgrad: Cin <= 32; the one-sweep backward: Cin = 16) */
int sc_head_conv_fwd(const sc_src* in, const float* w /*[1][Cin][3][3]*/, const float* bias,
                     float* out, int N, int Cin, int H, int W, sc_stream stream);
/* HOST: the kernel sc_head_conv_fwd launches for (Cin, width, 16-byte alignment of in->x, of out): the generic kernel (8 x 32 tiles,
 * any Cin) unless Cin == 16; for Cin == 16 the register-blocked 16 x 64 tile with 16-byte staging and stores when W % 4 == 0 and both
 * pointers are aligned (k_head_fwd16v), else with 4-byte staging (k_head_fwd16).  SC_ERR_ARG for Cin outside [1,32] or W < 1.  The
 * entry point dispatches on this value. */
enum sc_head_kernel { SC_HEAD_K_GENERIC = 0, SC_HEAD_K_FWD16 = 1, SC_HEAD_K_FWD16V = 2 };
int sc_head_fwd_kernel(int Cin, int W, int in_aligned16, int out_aligned16);
/* K-class head, 1 <= K <= 8, Cin <= 32, same source modes (RAW / AFFINE, no upsample): smp.Unet(classes=K) followed by
 * torch.argmax(dim=1).type(uint8) (starcop/sentinel2/models.py:63-78; classes = settings.model.num_classes,
 * models/model_module.py:244-251).  At least one of logits / classes is non-NULL; with logits == NULL no logit is stored.  classes
 * follows torch.argmax: the first maximal index wins, a NaN counts as maximal and the first NaN wins.  K == 1 forwards to
 * sc_head_conv_fwd (classes, if asked for, are zeros). */
int sc_head_conv_fwd_k(const sc_src* in, const float* w /*[K][Cin][3][3]*/, const float* bias /*[K]*/,
                       float* logits /*[N][K][H][W] or NULL*/, uint8_t* classes /*[N][H][W] or NULL*/,
                       int N, int Cin, int K, int H, int W, sc_stream stream);
int sc_head_conv_dgrad(const float* dlogits, const float* w, float* gin,
                       int N, int Cin, int H, int W, sc_stream stream);
size_t sc_head_wgrad_workspace_floats(int N, int Cin, int H, int W);
int sc_head_conv_wgrad(const float* dlogits, const sc_src* in, float* part, size_t part_floats,
                       float* dw, float* dbias, int N, int Cin, int H, int W, sc_stream stream);
/* dgrad + wgrad + dbias of the head in ONE sweep over (dlogits, in) -- Cin = 16 only (model_module.py:244-251: the decoder's last
 * block has 16 channels); same results as the two calls above, gin = gradient w.r.t. the ACTIVATED input.  Workspace as for
 * sc_head_conv_wgrad. */
/* bn_sums != NULL (then `in` must be the SC_SRC_AFFINE source of a BatchNorm'd tensor): the launch also leaves what
 * sc_bn_bwd_reduce(gin, in->x, in->cst, in->act, ...) would compute in a pass of its own over both tensors -- rows
 * bn_sums[sc_head_bwd_bn_rows(N, H, W)][Cin][2] = {sum g', sum g' x_hat} for sc_bn_bwd_finalize, and (bn_absmax != NULL, zeroed by
 * the caller) the range hint max |scale_c g'| -- because gin is that tensor's complete gradient and its values stream through
 * this kernel anyway. */
int sc_head_bwd_bn_rows(int N, int H, int W);
int sc_head_conv_bwd(const float* dlogits, const sc_src* in, const float* w, float* gin, float* part, size_t part_floats,
                     float* dw, float* dbias, int N, int Cin, int H, int W, double* bn_sums, float* bn_absmax, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* BatchNorm2d bookkeeping (torch.nn.BatchNorm2d inside smp/torchvision blocks)
 * training=1: batch statistics from the `nrows` partial rows of `stats` (count = N*H*W), running stats updated with
 *             `momentum` (unbiased variance), cst_fwd = {scale, shift, mean, invstd,...}
 * training=0: cst_fwd from running stats */
int sc_stat_rows(int kind, int N, int H, int W);
/* scratch (optional, SC_BN_FINALIZE_SCRATCH_DOUBLES(C) doubles): with >= 4096 rows the rows of all channels are first summed as
 * one coalesced stream into 64 fp64 partial rows there (the per-channel walk reads a 64-byte sector per 8 useful bytes) */
#define SC_BN_FINALIZE_SCRATCH_DOUBLES(C) (64 * 2 * (size_t)(C))
/* act_bound (optional, training=1): device float raised (order-independent atomic max; never lowered) to
 * max_c |gamma_c| sqrt(count - 1) + |beta_c| -- no normalised sample of `count` can exceed sqrt(count - 1), so this bounds every
 * |BatchNorm output| of the tensor BY CONSTRUCTION; the SC_TERMS_F16X2 kernels derive their activation scale from it (xbound).
 * The value written lies in [b, b (1 + 2^-22)] for that b (count = 1: sqrt(0), the bound is max |beta_c|). */
int sc_bn_finalize(const float* stats, int nrows, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps,
                   int training, float* cst_fwd, int C, double* scratch, float* act_bound, sc_stream stream);
/* HOST: the launch form of sc_bn_finalize for (rows, channels, scratch given, training): EVAL = constants from the running statistics
 * (k_bn_finalize<4>, no row is read); ROWS4 = below 4096 rows, 256 threads per channel; from 4096 rows up PRE64 = the coalesced
 * pre-reduction into 64 fp64 rows (scratch given and 2 C <= 1024) and else ROWS16 = 1024 threads per channel.  SC_ERR_ARG for C < 1,
 * or nrows < 1 in training.  The entry point dispatches on this value. */
enum sc_bn_finalize_form { SC_BN_FIN_EVAL = 0, SC_BN_FIN_ROWS4 = 1, SC_BN_FIN_ROWS16 = 2, SC_BN_FIN_PRE64 = 3 };
int sc_bn_finalize_form(int nrows, int C, int has_scratch, int training);
/* HOST: the launch form of sc_bn_bwd_finalize_rows32: PRE64 = the same pre-reduction (from 4096 rows, scratch given, 2 C <= 1024), else
 * ROWS_F32 = the float rows summed per channel.  SC_ERR_ARG for a non-positive size.  The entry point dispatches on this value. */
enum sc_bn_bwd_rows32_form { SC_BN_ROWS_F32 = 0, SC_BN_ROWS_PRE64 = 1 };
int sc_bn_bwd_rows32_form(int nrows, int C, int has_scratch);
/* HOST: the loop form of the streaming kernels over [N][C][HW] planes -- sc_add_srcs_absmax, sc_bn_bwd_reduce, sc_bn_bwd_small: VEC4 =
 * 16-byte loads (HW % 4 == 0 and every tensor the launch touches 16-byte aligned: aligned16 is that test, made by the entry point on
 * the OR of its pointers), else SCALAR = 4-byte loads.  SC_ERR_ARG for HW < 1.  The form changes how the elements are loaded, not what
 * is computed from them nor, within a form, the order of the sums. */
enum sc_ew_vec_form { SC_EW_SCALAR = 0, SC_EW_VEC4 = 1 };
int sc_ew_vec_form(int HW, int aligned16);
/* sums[row][C][2] = { sum g_bn, sum g_bn * xhat } over the row's pixels, g_bn = g * act'(BN(y));
 * rows = sc_stat_rows(SC_STAT_BNBWD, N, H, W).
 * absmax (optional, device float, zeroed by the caller before the first launch of a step): raised to
 * max_c |gamma_c * invstd_c| * max |g_bn| by an order-independent atomic max -- the range hint of the SC_TERMS_F16X2 kernels.
 * act_absmax (optional, device float, NEVER lowered -- a sticky record): raised to max |act(BN(y))|, the largest activation
 * value a consumer of this tensor stages; the two-fp16-term kernels need it below 32752 (HyperStarcopUNet.split_range_report) */
int sc_bn_bwd_reduce(const float* g, const float* y, const float* cst_fwd, int act,
                     double* sums, int N, int C, int HW, float* absmax, float* act_absmax, sc_stream stream);
/* dgamma, dbeta and the SC_SRC_BNBWD constants {scale, shift, A, B, D}  (sc_bn_bwd_finalize_rows32: float rows, sc_bnr_args) */
int sc_bn_bwd_finalize(const double* sums, int nrows, double count, const float* cst_fwd,
                       float* dgamma, float* dbeta, float* cst_bwd, int C, sc_stream stream);
int sc_bn_bwd_finalize_rows32(const float* rows, int nrows, double count, const float* cst_fwd,
                       float* dgamma, float* dbeta, float* cst_bwd, int C, double* scratch /* 64 * 2 * C doubles or NULL: coalesced pre-reduction from 4096 rows up */, sc_stream stream);
/* both steps in one launch for few-pixel layers (one block per channel over all N*HW elements); same outputs */
int sc_bn_bwd_small(const float* g, const float* y, const float* cst_fwd, int act, int N, int C, int HW,
                    float* dgamma, float* dbeta, float* cst_bwd, float* absmax, float* act_absmax, sc_stream stream);
/* out = v(a) + v(b)   (residual add of an inverted-residual block; b may be NULL) */
int sc_add_srcs(const sc_src* a, const sc_src* b, float* out, int N, int C, int HW, sc_stream stream);
/* `waiter` does not run anything queued after this call before everything queued on `signaller` up to this call has finished
 * (both streams of the SAME device; the calling thread owns both).  What torch.cuda.Stream.wait_stream does, with an event created
 * with hipEventDisableTiming | hipEventDisableSystemFence: no system-scope cache write-back at the fork / join points of the
 * weight-gradient stream (HyperStarcopUNet's backward, the counterpart of autograd's multi-stream backward under
 * starcop/models/model_module.py:69-88).  Not for ordering against the host or another device. */
int sc_stream_wait_stream(sc_stream waiter, sc_stream signaller);

/* same, and *absmax (device float, never lowered) is raised to max |out|: the range evidence for residual sums that feed a
 * two-fp16-term convolution without a BatchNorm in between (smp skip connections taken after an inverted-residual add).
 * out may be NULL (b too): then the call only records max |v(a)| -- the inference-time range check of a BatchNorm'd tensor */
int sc_add_srcs_absmax(const sc_src* a, const sc_src* b, float* out, int N, int C, int HW, float* absmax, sc_stream stream);
/* out[n,c,y,x] (+)= sum of the 2x2 block of in (backward of nearest x2 upsample) */
int sc_downsum2x2(const float* in, float* out, int accum, int N, int C, int Hout, int Wout,
                  sc_stream stream);
/* the two resampling ops of the reference's in-repo UNet (starcop/models/architectures/unet.py:15,35-43), each reading its input
 * through the source's prologue (bias + ReLU of the producing convolution):
 *   sc_maxpool2x2          : nn.MaxPool2d(2)            in [N,C,2*Hout,2*Wout] -> out [N,C,Hout,Wout]
 *   sc_upsample_bilinear2x : F.interpolate(scale_factor=2, mode='bilinear', align_corners=True)   in [N,C,Hin,Win] -> out [N,C,2Hin,2Win] */
int sc_maxpool2x2(const sc_src* in, float* out, int N, int C, int Hout, int Wout, sc_stream stream);
int sc_upsample_bilinear2x(const sc_src* in, float* out, int N, int C, int Hin, int Win, sc_stream stream);
/* their backward passes (autograd of the same two torch ops):
 *   sc_maxpool2x2_bwd          : gin[window] (+)= gpool at the FIRST maximum of each 2x2 window of v(in) (row-major order, as
 *                                max_pool2d_with_indices), 0 elsewhere;  in [N,C,2Hout,2Wout], gpool [N,C,Hout,Wout]
 *   sc_upsample_bilinear2x_bwd : gin [N,C,Hin,Win] = transpose of the interpolation applied to gout [N,C,2Hin,2Win]; a gather
 *                                with the forward weights (deterministic, no atomics)                                       */
int sc_maxpool2x2_bwd(const sc_src* in, const float* gpool, float* gin, int accum, int N, int C, int Hout, int Wout,
                      sc_stream stream);
int sc_upsample_bilinear2x_bwd(const float* gout, float* gin, int N, int C, int Hin, int Win, sc_stream stream);
int sc_fill_f64(double* p, double v, size_t n, sc_stream stream);
int sc_apply_src(const sc_src* a, float* out, int N, int C, int HW, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* loss (starcop/models/model_module.py:53-58,76-79): BCEWithLogits(pos_weight) * weight -> mean
 *   loss_sum : double[1] (zeroed by caller) accumulates sum of per-pixel weighted loss
 *   dlogits  : grad of mean(loss*weight) w.r.t. logits  (may be NULL)
 *   loss_px  : per-pixel unweighted loss (may be NULL)  */
int sc_bce_logits_weighted(const float* logits, const float* target, const float* weight,
                           float pos_weight, size_t n, double* loss_sum, float* dlogits,
                           float* loss_px, sc_stream stream);

/* Adam (torch.optim.Adam defaults, model_module.py:174): one fused pass over flat buffers.
 * bias corrections are computed on the host from the step count. */
int sc_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                 float lr, float beta1, float beta2, float eps, float weight_decay,
                 float bias_correction1, float bias_correction2_sqrt, float grad_scale,
                 const float* hp_dev /* optional device {lr, bc1, bc2_sqrt}: overrides the host values */,
                 sc_stream stream);
/* step[0] += 1 (device int64); hp_dev = {lr_dev[0], 1-beta1^step, sqrt(1-beta2^step)}: lets a captured
 * hipGraph replay the optimiser step with the right bias corrections and a scheduler-driven lr */
int sc_adam_prepare(int64_t* step, const float* lr_dev, float beta1, float beta2, float* hp_dev,
                    sc_stream stream);

/* masks (model_module.py:124,193-212,268-269):
 *   prediction = sigmoid(logits); pred_binary = ge0 ? logits>=0 : sigmoid>0.5   (int64)
 *   differences = 2*pred_binary + (target==1) (int64, if target)
 *   tile_count[n] = sum pred_binary (int64, zeroed by caller);
 *   then sc_pred_classification: cls[n] = count > 10*H*W/64^2 */
int sc_threshold_masks(const float* logits, const float* target, int ge0, float* prediction,
                       int64_t* pred_binary, int64_t* differences, int64_t* tile_count,
                       int N, int HW, sc_stream stream);
int sc_pred_classification(const int64_t* tile_count, int64_t* cls, int N, int H, int W,
                           sc_stream stream);

/* ------------------------------------------------------------------------- */
/* mag1c matched filters (starcop/models/mag1c.py: rmf :284-348, acrwl1mf :177-280), one work-group per
 * group of pixels (a detector column / column block: func_by_groups :116-174, mag1c_emit.py:58-84).
 * Pixels of a group are packed band-major: element (s, p) of group g is x[xoff[g] + s*Ppad[g] + p].
 * All statistics, the Cholesky factorisation and the per-pixel filter run in fp64 whatever the element type.
 * The covariance of the target-removed data is formed from the fixed scatter matrix of the group by the exact
 * rank-2 identity  N*C_k = C_0 - v t^T - t v^T + q t t^T  (see DESIGN.md), so X is streamed, never re-multiplied. */
typedef struct sc_mag1c_args {
  const void* x;            /* packed groups (see above)                                                  */
  int32_t x_is_f64;         /* element type of x / mf_out / albedo_out: 0 f32, 1 f64                      */
  const int64_t* xoff;      /* [G] element offsets of each group in x                                     */
  const int32_t* P;         /* [G] pixels per group                                                       */
  const int32_t* Ppad;      /* [G] row pitch (elements)                                                   */
  const int64_t* poff;      /* [G] offsets of each group in the per-pixel arrays                          */
  const uint8_t* statmask;  /* optional per-pixel (packed order) mask of pixels that enter mean/covariance */
  int32_t G, S;             /* groups, bands (S <= 128)                                                   */
  int64_t npix;             /* total packed pixels (sum of P)                                             */
  const double* templ;      /* [S] unit absorption spectrum                                               */
  int32_t num_iter;         /* reweighted-L1 iterations; -1: plain rmf()                                  */
  double alpha;             /* covariance shrinkage towards its diagonal (lerp)                           */
  double cov_update_scaling;
  int32_t albedo_override, zero_override, sparse_override, apply_scaling;
  double* work;             /* scratch: sc_mag1c_workspace_doubles(G, S, npix)                            */
  void* mf_out;             /* [npix] per-pixel outputs, element type of x                                */
  void* albedo_out;         /* [npix]                                                                     */
  int32_t* status;          /* [G] 0 ok, 1 covariance not positive definite (-> torch.linalg.LinAlgError), 2 see DIRECT mode */
  /* compute_energy of the reference (starcop/models/mag1c.py:270-275, 337-343), both null or both set:
   * energy [G][max(num_iter,0)+1] = sum of all entries of (x-mu) C_k^{-1} (x-mu)^T per group and iteration (entry 0: the rmf stage),
   * logdet [G] = P/2 * log(1 / prod diag chol C) of the rmf stage */
  double* energy;
  double* logdet;
  /* DIRECT mode (cube != NULL; fp32, S > 64, no energy, every group of at most 512 pixels -- a 512-row tile filtered per detector
   * column, func_by_groups at starcop/models/mag1c.py:116-174): the groups' pixels are read straight from the pixel-major cube through
   * pix_index (element (s, p) of group g = cube[pix_index[poff[g] + p] * S_total + band0 + s]) into the kernel's register tile, which
   * holds them for all iterations, and the results go straight to image order (scatter_mf / scatter_alb[pix_index[..]], element type
   * scatter_is_f64) -- no sc_mag1c_pack pass (one write + one read of the whole tile), no sc_scatter launches.  x / xoff / Ppad /
   * mf_out / albedo_out are unused (may be NULL); a group with P > 512 gets status 2. */
  const float* cube;
  int32_t S_total, band0;
  const int64_t* pix_index;
  void* scatter_mf; void* scatter_alb;
  int32_t scatter_is_f64;
} sc_mag1c_args;
size_t sc_mag1c_workspace_doubles(int G, int S, int64_t npix);
int sc_mag1c_groups(const sc_mag1c_args* a, sc_stream stream);
/* The launch or pair of launches sc_mag1c_groups takes, a pure host function and the ONE place the rule is written (the entry point
 * switches on it).  Arguments: what the dispatch depends on -- the band count, the element type of x, alpha == 0, compute_energy
 * (energy != NULL), DIRECT mode (cube != NULL).  Codes: 1000 + 100 * (JB / 4) + 10 * form + shrink for k_mag1c_tile<JB, RES, SHRINK,
 * ENERGY> on fp32 radiances (form 0: the streaming kernel alone, 1: the streaming energy kernel, 2: the resident + streaming pair,
 * 3: the resident kernel alone; shrink = alpha != 0), 2000 + 100 * (NT / 512) + 10 * energy for k_mag1c<double, NT, ENERGY> (fp64,
 * alpha != 0), 2000 for k_mag1c_fast<double, 1024> (fp64, alpha == 0).  JB = 4 / NT = 512 up to 64 bands, JB = 8 / NT = 1024 above.
 * k_mag1c_fast is ONE instantiation with and without compute_energy (a run-time branch on energy != NULL inside it), so both give
 * SC_MAG1C_F64_FAST.  SC_ERR_ARG with sc_last_error set for what sc_mag1c_groups refuses: S outside [1, 128]; DIRECT mode with fp64
 * radiances, with S <= 64 or with compute_energy. */
enum sc_mag1c_launch {
  SC_MAG1C_TILE4 = 1100, SC_MAG1C_TILE4_SHRINK = 1101,                 /* k_mag1c_tile<4, false, SHRINK>                             */
  SC_MAG1C_TILE4_ENERGY = 1110, SC_MAG1C_TILE4_ENERGY_SHRINK = 1111,   /* k_mag1c_tile<4, false, SHRINK, true>                       */
  SC_MAG1C_TILE8_ENERGY = 1210, SC_MAG1C_TILE8_ENERGY_SHRINK = 1211,   /* k_mag1c_tile<8, false, SHRINK, true>                       */
  SC_MAG1C_TILE8_PAIR = 1220, SC_MAG1C_TILE8_PAIR_SHRINK = 1221,       /* k_mag1c_tile<8, true, SHRINK> then <8, false, SHRINK>      */
  SC_MAG1C_TILE8_DIRECT = 1230, SC_MAG1C_TILE8_DIRECT_SHRINK = 1231,   /* k_mag1c_tile<8, true, SHRINK> alone, DIRECT mode           */
  SC_MAG1C_F64_FAST = 2000,                                            /* k_mag1c_fast<double, 1024>                                 */
  SC_MAG1C_F64_512 = 2100, SC_MAG1C_F64_512_ENERGY = 2110,             /* k_mag1c<double, 512, ENERGY>                               */
  SC_MAG1C_F64_1024 = 2200, SC_MAG1C_F64_1024_ENERGY = 2210            /* k_mag1c<double, 1024, ENERGY>                              */
};
int sc_mag1c_variant(int S, int x_is_f64, int alpha_is_zero, int energy, int direct);
/* gather the pixels of a (H,W,S_total) band-interleaved cube into the packed band-major layout:
 * x[xoff[g] + s*Ppad[g] + p] = cube[pix_index[poff[g]+p]*S_total + band0 + s] */
int sc_mag1c_pack(const void* cube, int cube_is_f64, int S_total, int band0, int S,
                  const int64_t* pix_index, const int64_t* xoff, const int32_t* Ppad,
                  const int64_t* poff, const int32_t* P, int G, void* xpacked, int out_is_f64,
                  sc_stream stream);
/* out[pix_index[i]] = val[i]  (results back to image order; fill the rest before calling) */
/* valid[p] = all(cube[p][band0 .. band0+S) > nodata): the default pixel mask of func_by_groups
 * (starcop/models/mag1c.py:140-142, torch.all(x > NODATA, dim=-1)) in one pass over the pixel-major cube */
int sc_valid_mask(const void* cube, int cube_is_f64, int S_total, int band0, int S, double nodata, int64_t npix,
                  unsigned char* valid, sc_stream stream);
int sc_scatter(const void* val, int val_is_f64, const int64_t* pix_index, size_t n, void* out,
               int out_is_f64, sc_stream stream);
/* same with the element count in device memory (n_dev[0] <= n_max): no host synchronisation between layout and scatter */
int sc_scatter_n(const void* val, int val_is_f64, const int64_t* pix_index, const int64_t* n_dev, size_t n_max, void* out,
                 int out_is_f64, sc_stream stream);
/* valid[p] = all(cube[p][band0 .. band0+S) != fill): the EMIT driver's pixel mask (starcop/models/mag1c_emit.py:60-66,
 * torch.any(raw == fill_value, dim=-1) inverted) in one pass over the pixel-major cube */
int sc_valid_mask_ne(const void* cube, int cube_is_f64, int S_total, int band0, int S, double fill, int64_t npix,
                     unsigned char* valid, sc_stream stream);
/* Packed layout of COLUMN-STRUCTURED groups, built on the device with no sort and no host round trip.  Both drivers of the
 * reference group by detector columns: one column per group in starcop/process_aviris.py:209-219 (un-orthorectified cubes),
 * blocks of column_step columns in starcop/models/mag1c_emit.py:58-84.  Group g = columns [gcol[g], gcol[g+1]) of a
 * (rows, cols) image; its pixels are the valid ones (valid[r*cols + c] != 0) in row-major order -- the order of the
 * reference's boolean indexing; a group with <= min_keep valid pixels gets P[g] = 0 and is skipped by sc_mag1c_groups
 * (starcop/models/mag1c.py:166: groups of <= 10 pixels are not filtered).
 * Outputs (device): P[G], Ppad[G] (P rounded up to 64), poff[G] / xoff[G] (exclusive scans of P and of Ppad*S),
 * pix_index[rows*cols] (the first sum(P) entries are written), totals[2] = {sum P, sum Ppad*S}. */
int sc_mag1c_layout_columns(const unsigned char* valid, int rows, int cols, const int32_t* gcol /*[G+1]*/, int G, int S,
                            int min_keep, int32_t* P, int32_t* Ppad, int64_t* poff, int64_t* xoff, int64_t* pix_index,
                            int64_t* totals, sc_stream stream);

/* The same packed layout for ARBITRARY integer groups -- the orthorectified AVIRIS-NG cube, where the group of a pixel is
 * |GLT sample index| (starcop/process_aviris.py:211-217: samples_glt_file = abs(glt[..., 0]), 0 = no data), ids bounded by the
 * detector width: a stable counting sort on the device (per-1024-pixel-block histograms, a scan over the blocks per id, ranked
 * scatter) instead of torch.nonzero / argsort / unique_consecutive / repeat_interleave and their host round trip.
 * Group g = id value g in [0, nids): its pixels are the valid ones (valid[p] != 0, ids[p] == g) in ascending pixel index (the
 * order of the reference's boolean indexing x[groups == g]); ids outside [0, nids) are ignored; a group with <= min_keep valid
 * pixels gets P[g] = 0.  Outputs as sc_mag1c_layout_columns with G = nids; work: sc_mag1c_layout_ids_workspace_ints ints. */
size_t sc_mag1c_layout_ids_workspace_ints(int64_t npix, int nids);
int sc_mag1c_layout_ids(const unsigned char* valid, const int32_t* ids, int64_t npix, int nids, int S, int min_keep,
                        int32_t* P, int32_t* Ppad, int64_t* poff, int64_t* xoff, int64_t* pix_index, int64_t* totals,
                        int32_t* work, sc_stream stream);

/* band-ratio feature (starcop/data/feature_extration.py:37-56).  For B tiles of n pixels:
 *   sc_trimmed_sums : sums[b] = sum of x[b][i] with lower <= x <= upper, lower/upper = numpy.percentile(x[b], p / 100-p)
 *                     (exact order statistics by radix select + numpy's linear interpolation)   == np.sum(no_outliers(x, p))
 *   sc_band_ratio   : R = (c*signal - background)/(background + 1e-6), c = sum_bg/sum_sig per tile (device sums) or c_host;
 *                     pixels with signal < 1e-6 and background < 1e-6 get zero_value_out                                    */
size_t sc_trimmed_sum_workspace_bytes(int B);
int sc_trimmed_sums(const float* x, int B, size_t n, double p, double* sums, void* work, size_t work_bytes,
                    sc_stream stream);
int sc_band_ratio(const float* background, const float* signal, float* out, int B, size_t n,
                  const double* sum_bg, const double* sum_sig, float c_host, float zero_value_out,
                  sc_stream stream);
/* out = clip(x/div, lo, hi) * mult (+ nan_to_num): weight_mag1c (feature_extration.py:32-35: div 400, clip [0.1,1], mult 1)
 * and the EMIT->AVIRIS rescale (emit_tools/emit_dataset.py:62-106: mf/240 -> [0,2] * 1750, rgb/20 -> [0,2] * 60) */
int sc_clip_scale(const float* x, float* out, size_t n, float div, float lo, float hi, float mult,
                  int nan_to_num, sc_stream stream);

/* Sanchez-Garcia multiple-linear-regression ratio (starcop/data/feature_extration.py:58-125, ratio_MLR_local and its
 * _5IN / _9IN / _5IN_simplediv wrappers).  For B tiles of n pixels: the least-squares fit with intercept of the target band t
 * on k <= 9 regressor bands x_1..x_k over ALL pixels (sklearn LinearRegression), r = intercept + sum_j coef_j x_j, then
 *   SC_MLR_C_MATCHED   : R = (c*r - t)/(t + 1e-6), c = trimmed sum(t) / trimmed sum(r) (sc_trimmed_sums, p = 5, float32
 *                        division as sc_band_ratio); -0.5 where (r < 1e-6 and t < 1e-6) or t == 0
 *   SC_MLR_SIMPLE_PLUS : R0 = -t/(r + 1e-6), R = (R0 - mean(R0))/std(R0) (ddof 0, fp64 over the tile); min(R) where t == 0
 *   SC_MLR_RESIDUAL    : R = (t - r)/(r + 1e-6); 0 where t == 0
 * and with autoclip != 0, R = clip(R, -0.2, 0.2).
 * Regressor j of tile b is the plane base + b*tile_stride + band_off[j] and the target of tile b is target + b*target_tile_stride
 * (offsets and strides in floats), so a stacked (B, bands, H, W) tensor is used in place.
 *   sc_mlr_moments : fp64 sums of z and z z^T (z = [x, t] minus a per-band shift) into per-work-group partials of `work`
 *   sc_mlr_solve   : fixed-order reduction of those partials, equilibrated fp64 Jacobi eigen-solve, minimum-norm solution;
 *                    coef[b][0..k-1] = coefficients (0 for a zero-variance band), coef[b][k] = intercept (fp64, device)
 *   sc_mlr_fit     : sc_mlr_moments + sc_mlr_solve
 *   sc_mlr_predict : r[b][i] (dense [B][n] fp32) from coef
 *   sc_mlr_ratio   : out[b][i] (dense [B][n] fp32) from coef and t; SC_MLR_C_MATCHED also reads r (sc_mlr_predict), the other
 *                    divisions evaluate r in fp64 themselves and take r = NULL
 * No atomics: repeated calls give bit-identical results.  work: sc_mlr_workspace_bytes(B, n, k) bytes.              */
enum sc_mlr_division { SC_MLR_C_MATCHED = 0, SC_MLR_SIMPLE_PLUS = 1, SC_MLR_RESIDUAL = 2 };
typedef struct sc_mlr_args {
  const float* base;             /* regressor planes                                    */
  long long band_off[16];        /* offset of regressor j from base, floats (j < k)     */
  int32_t k;                     /* regressors, 1..9                                    */
  long long tile_stride;         /* floats between tiles of the regressors              */
  const float* target;           /* target plane of tile 0                              */
  long long target_tile_stride;  /* floats between tiles of the target                  */
  int32_t B;                     /* tiles                                               */
  size_t n;                      /* pixels per tile (H*W, any value >= 2)               */
} sc_mlr_args;
size_t sc_mlr_workspace_bytes(int B, size_t n, int k);
int sc_mlr_moments(const sc_mlr_args* a, void* work, size_t work_bytes, sc_stream stream);
int sc_mlr_solve(const sc_mlr_args* a, double* coef, void* work, size_t work_bytes, sc_stream stream);
int sc_mlr_fit(const sc_mlr_args* a, double* coef, void* work, size_t work_bytes, sc_stream stream);
int sc_mlr_predict(const sc_mlr_args* a, const double* coef, float* r, sc_stream stream);
int sc_mlr_ratio(const sc_mlr_args* a, const double* coef, const float* r, int division, int autoclip, float* out, void* work, size_t work_bytes,
                 sc_stream stream);

/* Connected-component labelling and the plume label masks (starcop/data/mask_creation.py:6-27 proposed_mask, called by
 * WindowDataset at sampling_dataset.py:298-303 and cached as labelbinary.tif by _cache_data_permian_2019 :453-460).
 *   sc_proposed_mask        : for each of N images, T = mag1c >= threshold (NaN unset), D = dilation(opening(T)) with the 3x3
 *                             element se_bits (SC_SE_CROSS = skimage disk(1); erosion: outside the image set, dilations: outside
 *                             unset -- skimage's binary_erosion / binary_dilation borders; se_bits = 0: D = T), components of D
 *                             with 8-connectivity (skimage.measure.label's default), out[n][h][w] (uint8) = T & D & (the
 *                             component of the pixel holds a pixel with alpha != 0).  mag1c plane n = mag1c + n*mag1c_plane_stride
 *                             and alpha plane n = alpha + n*alpha_plane_stride (elements; dense H x W planes), so channel 3 of a
 *                             (N, 4, H, W) label_rgba tensor is read in place.
 *   sc_connected_components : labels[n][h][w] (int32) of mask != 0, connectivity 1 (4-neighbours) or 2 (8-neighbours); background
 *                             0, components numbered 1.. by their first pixel in raster order (scipy.ndimage.label /
 *                             skimage.measure.label); counts[n] = number of components (device int32).
 * Union-find: a per-tile pass in LDS, a border merge with device atomics, a flatten; the root of a component is its minimum
 * raster index, so repeated calls give identical bits.  4 (proposed_mask) / 5 (connected_components) launches per call.
 * N <= 65535, H*W < 2^31.  work: sc_label_workspace_bytes(N, H, W) bytes (enough for either).                    */
size_t sc_label_workspace_bytes(int N, int H, int W);
int sc_connected_components(const uint8_t* mask, int connectivity, int32_t* labels, int32_t* counts,
                            void* work, size_t work_bytes, int N, int H, int W, sc_stream stream);
int sc_proposed_mask(const float* mag1c, int64_t mag1c_plane_stride, const uint8_t* alpha, int64_t alpha_plane_stride,
                     float threshold, int se_bits, uint8_t* out, void* work, size_t work_bytes,
                     int N, int H, int W, sc_stream stream);

/* Simulated multispectral bands from an AVIRIS-NG radiance cube: the spectral-response-function resampling of
 * starcop/data/aviris.py:262-331 (transform_to_srf; the weights of :288-312, the sum and fill mask of :318-327), which
 * starcop/process_aviris.py:26-90 (aviris_as_sensor) runs once per WorldView-3 / Sentinel-2 band and per 50-column window.
 *   sc_srf_bands : out[j][l][s] = sum over k in support(j) of w[k] * x[l][s][band[k]] for every output band j < n_out in one launch;
 *                  each product in fp64 (float32 value promoted exactly), added in ascending band order onto a +0.0 seed,
 *                  rounded once to float32 -- bit-equal to numpy's np.sum(w[:, None, None] * x_stack, axis=0).  With
 *                  has_fill, out[j][l][s] = fill where any support value equals fill (float32 comparison).
 * Cube element (l, s, b) = x[l*line_stride + s*sample_stride + b*band_stride] (elements, >= 0): ENVI BIP / BIL / BSQ memmap chunks
 * and permuted tensor views are read in place; only the band window [min band, max band] of the CSR is read.  Output plane j,
 * line l starts at out + j*out_plane_stride + l*out_line_stride (samples dense), so a chunk can land at a line offset of a whole
 * flight-line buffer.  The weights are CSR rows (ptr[n_out + 1], band[nnz] strictly ascending within a row, w[nnz] fp64) given
 * twice: on the device for the kernel, and ptr_host / band_host for the argument checks and the band window (no device read
 * back).  SC_ERR_ARG for bad dims, n_out outside [1, 64], an empty row, a band outside [0, B) or a row that is not ascending.
 * No atomics: repeated calls give identical bits.                                                                        */
typedef struct sc_srf_args {
  const float* x;              /* cube element (0, 0, 0)                                  */
  int64_t line_stride;         /* elements                                                */
  int64_t sample_stride;
  int64_t band_stride;
  int32_t L, S, B;             /* lines, samples, bands                                   */
  int32_t n_out;               /* output bands, 1..64                                     */
  const int32_t* ptr;          /* [n_out + 1] device                                      */
  const int32_t* band;         /* [nnz] device                                            */
  const double* w;             /* [nnz] device                                            */
  const int32_t* ptr_host;     /* the same ptr / band on the host                         */
  const int32_t* band_host;
  float* out;                  /* float32                                                 */
  int64_t out_plane_stride;    /* elements between output bands                          */
  int64_t out_line_stride;     /* elements between output lines                           */
  int32_t has_fill;
  float fill;
} sc_srf_args;
int sc_srf_bands(const sc_srf_args* a, sc_stream stream);

/* Anti-aliased downscaling of the simulated bands to the sensor's pixel size: the read.resize(..., anti_aliasing=True,
 * anti_aliasing_sigma=sigma_bands) that ends starcop/data/aviris.py:262-338 (transform_to_srf), which wraps
 * skimage.transform.resize(order=1, anti_aliasing=True) = per plane, scipy.ndimage.gaussian_filter followed by scipy.ndimage.zoom(order=1,
 * grid_mode=True).  That operator is separable and linear in (x, cval), so it is given here as tap tables per axis:
 *   sc_resize_aa : tmp[p][j][s] = f32( sum_k wy[j][k] * x_p[start_y[j] + k][s] + wcy[j] * cval )        (vertical pass, first)
 *                  out[p][j][i] = f32( sum_k wx[i][k] * tmp[p][j][start_x[i] + k] + wcx[i] * cval )      (horizontal pass)
 *                  each product in fp64 (float32 value promoted exactly), added in ascending tap order onto a +0.0 seed, the cval term
 *                  added last, no fused multiply-add, rounded once to float32 at the end of each pass -- bit-equal to a numpy loop over
 *                  the taps, identical between calls and between a plane alone and inside a batch.  No atomics.
 * Input plane p, element (l, s) = x[p*plane_stride + l*line_stride + s*sample_stride] (elements, >= 0): a permuted view or a line range
 * of a larger buffer is read in place.  Output plane p, line j starts at out + p*out_plane_stride + j*out_line_stride (samples dense).
 * An axis (sc_resize_axis) carries n_tables tap tables of o outputs: start[t][o] (first input sample of the window), w[t][o][T] (fp64,
 * rows zero-padded to the common row length T) and wc[t][o] (the weight that goes to cval); taps[t] <= T is the number of leading
 * entries of table t's rows that are used (NULL: T for every table).  Plane p uses table table_y[p] / table_x[p], so planes with equal
 * sigma share one.  start, taps and the plane -> table maps are given twice: on the device for the kernels, on the host for the checks
 * that run before anything is launched.  Downscaling only (o <= n; o == n is a blur, or the identity).
 * SC_ERR_ARG for bad dims, an output larger than the input, P outside [1, 65535], T outside [1, 256], a tap window that leaves [0, n),
 * a table index out of range, negative strides, null pointers or a workspace below sc_resize_workspace_bytes(P, oh, W) bytes (the
 * float32 intermediate).  Two launches per call, all planes in each.                                                            */
typedef struct sc_resize_axis {
  int32_t n, o;                /* input and output length of the axis, o <= n           */
  int32_t n_tables;
  int32_t T;                   /* row length of w, 1..256                               */
  const int32_t* start;        /* [n_tables][o] device                                  */
  const int32_t* taps;         /* [n_tables] device, or NULL                            */
  const double* w;             /* [n_tables][o][T] device                               */
  const double* wc;            /* [n_tables][o] device                                  */
  const int32_t* start_host;   /* the same start / taps on the host                     */
  const int32_t* taps_host;
} sc_resize_axis;
typedef struct sc_resize_args {
  const float* x;              /* element (0, 0) of plane 0, device                     */
  int64_t plane_stride;        /* elements                                              */
  int64_t line_stride;
  int64_t sample_stride;
  int32_t P;                   /* planes                                                */
  float cval;
  float* out;                  /* float32, device                                       */
  int64_t out_plane_stride;    /* elements between output planes                        */
  int64_t out_line_stride;     /* elements between output lines                         */
  sc_resize_axis y;            /* lines:   n = H, o = oh                                */
  sc_resize_axis xs;           /* samples: n = W, o = ow                                */
  const int32_t* table_y;      /* [P] device: table of every plane, per axis            */
  const int32_t* table_x;
  const int32_t* table_y_host; /* the same on the host                                  */
  const int32_t* table_x_host;
  void* work;                  /* device                                                */
  size_t work_bytes;
} sc_resize_args;
size_t sc_resize_workspace_bytes(int P, int oh, int W);
int sc_resize_aa(const sc_resize_args* a, sc_stream stream);

/* Window statistics of a mag1c flight line: the table scripts/preprocessing/stats_mag1c.py:24-70 writes (512 x 512 windows at
 * overlap 256) and starcop/data/sampling_dataset.py:112-179, 408-439 samples the no-plume windows from.
 *   sc_window_stats : for each of n_win windows (row_off, col_off, height, width; any sizes, any overlap, duplicates allowed) of one
 *                     float32 scene, over V = { min(v, clip_max) : v in window, v != fill (if has_fill), v >= 0 } (stats_mag1c.py:
 *                     45-48: NaN fails v >= 0, -0.0 passes, +inf becomes clip_max, a NaN fill masks nothing):
 *                       count[i]                 number of members (int64)
 *                       sum_mean[i][0..1]        sum and mean, accumulated in fp64
 *                       stats[i][0..6]           max, min, percentiles 1, 5, 50 (median), 95, 99 (float32)
 *                     Percentiles are numpy.percentile(method="linear") / numpy.median of the float32 values as numpy >= 2.0
 *                     evaluates them: virtual index float32(count - 1) * (float32(q) / float32(100)), the two neighbouring EXACT
 *                     order statistics a <= b, weight t = frac(index), a + (b - a) * t, or b - (b - a) * (1 - t) where t >= 0.5,
 *                     every operation rounded to float32; median = (a + b) / 2 of the two middle order statistics.  The sign of a
 *                     zero result is unspecified (-0.0 and +0.0 are equal keys).  count == 0: count 0, NaN everywhere else.
 * Scene element (r, c) = x[r*row_stride + c] (row_stride >= W elements): a column slice of a wider tensor is read in place, no
 * per-window copies.  The windows are given twice: on the device for the kernels, on the host for the argument check (every window
 * inside the scene, height and width >= 1) that runs before anything is launched.  H*W < 2^31, 1 <= n_win <= 2^20, clip_max >= 0.
 * All ten order statistics of a window are resolved together by an exact 3-pass radix select (11 + 10 + 10 bits of the non-
 * negative float bit patterns); integer histogram atomics only, the fp64 sums are added in a fixed order: repeated calls give
 * identical bits.  7 launches per call.  work: sc_window_stats_workspace_bytes(n_win) bytes (about 48 KiB per window).      */
typedef struct sc_winstats_args {
  const float* x;                /* scene element (0, 0), device                            */
  int64_t row_stride;            /* elements                                                */
  int32_t H, W;
  int32_t has_fill;
  float fill;
  float clip_max;
  int32_t n_win;
  const int32_t* windows;        /* [n_win][4] device                                       */
  const int32_t* windows_host;   /* the same on the host                                    */
  int64_t* count;                /* [n_win] device                                          */
  double* sum_mean;              /* [n_win][2] device                                       */
  float* stats;                  /* [n_win][7] device                                       */
} sc_winstats_args;
size_t sc_window_stats_workspace_bytes(int n_win);
int sc_window_stats(const sc_winstats_args* a, void* work, size_t work_bytes, sc_stream stream);

/* Orthorectification of EMIT products through the granule's geometry look-up table: what starcop/models/mag1c_emit.py:86-88
 * (ei.georreference(mag1c_output, fill_value_default=...) and the same on the albedo, the georreferenced=True default of
 * mag1c_emit) leaves in its outputs; the gather is restated in the note at mag1c_emit.py:206-221 (single_image_ortho).
 *   sc_glt_ortho : for P planes in one launch
 *                    out[p][i][j] = src_p[gy - 1][gx - 1]   if glt_x[i][j] != 0 and glt_y[i][j] != 0
 *                                   fill[p]                 otherwise
 *                  with (gx, gy) = (glt_x[i][j], glt_y[i][j]) (1-based column / row of the swath), or their absolute values when
 *                  `absolute` is set (AVIRIS-NG GLTs mark interpolated pixels with a negative index).
 * Pure data movement: elements are copied as words of elem_bytes (1, 2, 4 or 8; one width per call) and fill values are bit patterns
 * (the low elem_bytes of fill_bits[p]), so the result is bit-equal to the numpy gather for float32, float64, uint8, int16, int32,
 * .. including NaN payloads and -0.0.  Source plane p is read in place: element (r, c) = src[p] + (r*row_stride[p] +
 * c*col_stride[p]) elements, strides >= 0 -- a stacked (P, rows, cols) tensor is src[p] = base + p*plane_stride, a pixel-interleaved
 * (rows, cols, C) cube is src[p] = base + p with col_stride = C, lists of separate tensors and permuted views likewise.  A plane may
 * cover only the top-left plane_rows[p] x plane_cols[p] of the swath (0 = the whole swath): GLT entries beyond it give fill[p].
 * glt_x / glt_y: dense int32 [out_h][out_w]; out: dense [P][out_h][out_w].
 * A GLT entry that is not no-data and points outside the swath (gx > cols, gy > rows, or negative without `absolute`) is never
 * dereferenced: the pixel gets fill[p] in every plane and *oob_count (device, may be NULL; the caller zeroes it) is incremented once
 * per such pixel.  The two GLT words are read once per pixel; 16-byte stores when out_w * elem_bytes is a multiple of 16 and out /
 * glt_x / glt_y are 16-byte aligned.  SC_ERR_ARG for bad dims, P outside [1, 64], an unsupported elem_bytes, null or misaligned
 * pointers, negative strides, a plane extent outside the swath.  No other atomics: repeated calls give identical bits.          */
#define SC_ORTHO_MAX_PLANES 64
typedef struct sc_ortho_args {
  const int32_t* glt_x;                          /* [out_h][out_w] device: 1-based swath column, 0 = no data */
  const int32_t* glt_y;                          /* [out_h][out_w] device: 1-based swath row, 0 = no data    */
  int32_t out_h, out_w;
  int32_t rows, cols;                            /* the swath the GLT indexes                                 */
  int32_t P;                                     /* planes, 1..64                                             */
  int32_t elem_bytes;                            /* 1, 2, 4 or 8                                              */
  int32_t absolute;                              /* use |gx|, |gy|                                            */
  int32_t reserved;
  const void* src[SC_ORTHO_MAX_PLANES];          /* element (0, 0) of every plane, device                     */
  int64_t row_stride[SC_ORTHO_MAX_PLANES];       /* elements                                                  */
  int64_t col_stride[SC_ORTHO_MAX_PLANES];
  int32_t plane_rows[SC_ORTHO_MAX_PLANES];       /* extent of the plane inside the swath; 0 = rows / cols     */
  int32_t plane_cols[SC_ORTHO_MAX_PLANES];
  uint64_t fill_bits[SC_ORTHO_MAX_PLANES];       /* raw bit pattern of every plane's fill value               */
  void* out;                                     /* [P][out_h][out_w] device                                  */
  uint64_t* oob_count;                           /* device, or NULL                                           */
} sc_ortho_args;
int sc_glt_ortho(const sc_ortho_args* a, sc_stream stream);

/* Reprojection of rasters between grids (the warp), for P planes in one launch.  For every pixel (r, c) of the destination grid:
 *   (x, y) = dst_gt applied to the pixel centre (c + 0.5, r + 0.5)     [GDAL order: x = gt[0] + col*gt[1] + row*gt[2],
 *                                                                                   y = gt[3] + col*gt[4] + row*gt[5]]
 *   (x, y) : destination CRS -> source CRS.  CRS codes: equal codes on both sides (0 included) = same CRS, affine only; otherwise
 *            each side is 4326 (WGS-84 longitude / latitude, degrees) or 32601..32660 / 32701..32760 (WGS-84 UTM north / south).
 *            Transverse Mercator is the Krueger series to order n^6 (Karney 2011, alpha / beta coefficients), complex Clenshaw
 *            summation, the conformal latitude inverted with a fixed number of Newton steps; zone A -> zone B goes through
 *            longitude / latitude.  A point further than 30 degrees of longitude from the central meridian of a UTM side, a latitude
 *            beyond +-90 and a result that is not finite are outside the source.
 *   (u, v) = src_inv applied to (x, y): u = inv[0] + x*inv[1] + y*inv[2], v = inv[3] + x*inv[4] + y*inv[5] -- the inverse of the
 *            source's geotransform, inverted by the caller in float64 (so either side may be rotated); outside unless
 *            0 <= u < src_w and 0 <= v < src_h.
 *   SC_WARP_NEAREST  : out[p][r][c] = src_p[floor(v)][floor(u)], copied as a word of elem_bytes (1, 2, 4 or 8; one width per call);
 *                      nodata_bits[p] (its low elem_bytes) when outside -- bit-equal to a numpy gather for every dtype.
 *   SC_WARP_BILINEAR : float32 planes (elem_bytes = 4).  With fx = u - 0.5 - floor(u - 0.5) and fy likewise the four pixels around
 *                      (u - 0.5, v - 0.5) are weighed (1 - fx | fx) * (1 - fy | fy) in fp64; a sample counts when it lies inside the
 *                      raster, is not NaN and is not nodata_bits[p] (compared as bits) and has a weight > 0; the sum is divided by the
 *                      weight of the samples that count and rounded once to float32.  The pixel is nodata when it is outside or its
 *                      NEAREST source pixel does not count: both modes have the same valid pixels.
 * All of it in fp64, once per pixel and not once per plane.  Source plane p is read in place: element (row, col) = src[p] +
 * (row*row_stride[p] + col*col_stride[p]) elements, strides >= 0, every plane src_h x src_w.  out: dense [P][out_h][out_w].
 * coords (device, may be NULL): float64 [2][out_h][out_w], (u, v) of every pixel, NaN for "outside"; a call with P = 0 writes only
 * this.  *oob_count (device, may be NULL; the caller zeroes it) is incremented once per pixel outside the source.  16-byte stores
 * (4 float32 pixels per thread) when out_w is a multiple of 4 (2 for 8-byte elements) and out is aligned to the store.
 * SC_ERR_ARG for a null or misaligned pointer, P outside [0, 32] (0 only with coords), non-positive shapes, out_h*out_w >= 2^31, an
 * unsupported elem_bytes / resampling / CRS pair, bilinear on another width than 4, a negative stride, a singular or non-finite
 * geotransform.  No LDS, no other atomics: repeated calls give identical bits.                                                  */
#define SC_WARP_MAX_PLANES 32
#define SC_WARP_NEAREST 0
#define SC_WARP_BILINEAR 1
#define SC_WARP_UNBOUNDED 1   /* flags, coordinates-only calls: (u, v) outside the raster are written, NaN only where the projection fails */
typedef struct sc_warp_args {
  double dst_gt[6];                              /* geotransform of the destination grid, GDAL order           */
  double src_inv[6];                             /* world -> source pixel coordinates (see above)               */
  int32_t dst_crs, src_crs;                      /* 0, 4326, 326zz, 327zz                                      */
  int32_t out_h, out_w;
  int32_t src_h, src_w;
  int32_t P;                                     /* planes, 0..32                                              */
  int32_t elem_bytes;                            /* 1, 2, 4 or 8 (ignored with P = 0)                          */
  int32_t resampling;                            /* SC_WARP_NEAREST, SC_WARP_BILINEAR                          */
  int32_t flags;                                 /* SC_WARP_UNBOUNDED: P = 0 only                              */
  const void* src[SC_WARP_MAX_PLANES];           /* element (0, 0) of every plane, device                      */
  int64_t row_stride[SC_WARP_MAX_PLANES];        /* elements                                                   */
  int64_t col_stride[SC_WARP_MAX_PLANES];
  uint64_t nodata_bits[SC_WARP_MAX_PLANES];      /* raw bit pattern of every plane's no-data value             */
  void* out;                                     /* [P][out_h][out_w] device (NULL with P = 0)                 */
  double* coords;                                /* [2][out_h][out_w] device, or NULL                          */
  uint64_t* oob_count;                           /* device, or NULL                                            */
} sc_warp_args;
int sc_warp(const sc_warp_args* a, sc_stream stream);

/* Footprint resampling for the warp: where sc_warp looks at the destination pixel's CENTRE, this operator reduces every source pixel
 * under the destination pixel's FOOTPRINT -- what a coarser destination grid needs.  For destination pixel (r, c), in fp64:
 *   corners : (c, r), (c+1, r), (c, r+1), (c+1, r+1) go through the arithmetic of sc_warp's centre (dst_gt, the CRS route, src_inv),
 *             unclipped.  A corner without a finite result or outside the 30-degree band makes the pixel no-data.
 *   box     : u0 = min u_k, u1 = max u_k, v0, v1 likewise: the axis-aligned BOUNDING BOX of the footprint in source pixel
 *             coordinates (for a rotated pair larger than the true quadrilateral, as in GDAL).  A = (u1 - u0)(v1 - v0) is its
 *             unclipped area; it is clipped to [0, src_w] x [0, src_h] -> [cu0, cu1] x [cv0, cv1]; empty = no-data.
 *   weights : source column j in [floor(cu0), ceil(cu1)) has wx = min(j+1, cu1) - max(j, cu0), row i likewise wy.  A source pixel
 *             TAKES PART when wx > 2^-20 and wy > 2^-20 (the sliver rule: on a shared lattice with an integer ratio the corners land
 *             on integers +- 1e-11, and max / min / mode must not depend on that noise); its weight is w = wx * wy.
 *   counting: a taking-part sample COUNTS when it differs in bits from nodata_bits[p] and (float32) is not NaN.
 *   coverage: per plane, sum of w over counting samples / A.  The pixel is data when a sample counts and coverage >= min_coverage
 *             (all modes); otherwise nodata_bits[p] is written.
 *   SC_WARP_AREA_AVERAGE : float32.  sum w x / sum w over counting samples, rounded once.
 *   SC_WARP_AREA_MAX/MIN : float32 or uint8.  The extreme counting sample, exact bits (float32 in the total order -0 < +0; NaN
 *                          never counts, infinities do).
 *   SC_WARP_AREA_MODE    : uint8.  The value with the most counting samples (unweighted, integer tally), ties to the smallest.
 * coverage (device, may be NULL): float32 [P][out_h][out_w], the coverage where the pixel is data and 0 where it is no-data, so
 * that sum average * coverage * pixel area conserves an integral.  boxes (device, may be NULL): float64 [4][out_h][out_w] =
 * u0, u1, v0, v1 unclipped, NaN where a corner has no coordinates; a call with P = 0 writes only this.
 * A work-group projects the 17 x 17 (17 x 65 with 16-byte stores in the thread mapping) corners of its tile once into LDS -- about
 * 1.1 projections per pixel, not 4 -- and box, clip and weights are computed once per pixel for all planes.  Two mappings:
 *   variant 1 (thread)    : one thread per destination pixel loops over its box; for boxes of a few source pixels.
 *   variant 2 (lane group): 16 lanes own one destination pixel and run along source columns, the 4 groups of a wave own 4
 *                           adjacent pixels of a row, so a wave reads one contiguous segment per source row; the partial results
 *                           are combined by a fixed xor-butterfly (8, 4, 2, 1).  The mode tally is a 256-bin LDS histogram per group.
 *   variant 0             : chosen from the box width (source columns) of the destination grid's four corner pixels, estimated on
 *                           the host; sc_warp_area_variant returns that choice (1 or 2) or SC_ERR_ARG.
 * max / min / mode are bit-equal between the variants, average to the last place or two (another fp64 summation order).  Loops over
 * the box have no cap.  No floating-point atomics, a fixed reduction order: repeated calls give identical bits.  Planes are read in
 * place as in sc_warp; 16-byte stores (4-byte for uint8) when out_w is a multiple of 4 and out / coverage are aligned to them.
 * SC_ERR_ARG ("sc_warp_area: ...") as sc_warp, and for a mode / elem_bytes pair not listed above, min_coverage outside [0, 1] or
 * NaN, variant outside 0..2, P = 0 without boxes.                                                                                 */
#define SC_WARP_AREA_AVERAGE 2
#define SC_WARP_AREA_MAX 3
#define SC_WARP_AREA_MIN 4
#define SC_WARP_AREA_MODE 5
#define SC_WARP_AREA_THREAD 1
#define SC_WARP_AREA_LANES 2
typedef struct sc_warp_area_args {
  double dst_gt[6];                              /* geotransform of the destination grid, GDAL order           */
  double src_inv[6];                             /* world -> source pixel coordinates, as in sc_warp_args       */
  int32_t dst_crs, src_crs;                      /* 0, 4326, 326zz, 327zz                                      */
  int32_t out_h, out_w;
  int32_t src_h, src_w;
  int32_t P;                                     /* planes, 0..32 (0: boxes only)                              */
  int32_t elem_bytes;                            /* 4 = float32, 1 = uint8 (ignored with P = 0)                */
  int32_t mode;                                  /* SC_WARP_AREA_AVERAGE ... SC_WARP_AREA_MODE                 */
  int32_t variant;                               /* 0 = chosen by the library, SC_WARP_AREA_THREAD / _LANES    */
  double min_coverage;                           /* [0, 1]                                                     */
  const void* src[SC_WARP_MAX_PLANES];           /* element (0, 0) of every plane, device                      */
  int64_t row_stride[SC_WARP_MAX_PLANES];        /* elements                                                   */
  int64_t col_stride[SC_WARP_MAX_PLANES];
  uint64_t nodata_bits[SC_WARP_MAX_PLANES];      /* raw bit pattern of every plane's no-data value             */
  void* out;                                     /* [P][out_h][out_w] device (NULL with P = 0)                 */
  float* coverage;                               /* [P][out_h][out_w] device, or NULL                          */
  double* boxes;                                 /* [4][out_h][out_w] device, or NULL                          */
} sc_warp_area_args;
int sc_warp_area(const sc_warp_area_args* a, sc_stream stream);
int sc_warp_area_variant(const sc_warp_area_args* a);

/* Mosaic: N rasters on grids of their own composed into ONE raster on a destination grid, in one launch.  Per destination pixel the
 * world coordinates of the centre are computed once; when the destination is a UTM zone and a source of the pixel's tile has another
 * CRS, longitude / latitude (the Krueger inverse) once per pixel and not once per source; per source nothing more (same CRS), the
 * affine of longitude / latitude (4326) or the Krueger forward series (another zone; shared by consecutive sources of one code), then
 * that source's inverse affine -> (u, v), inside as in sc_warp.  All of it is the arithmetic of sc_warp (one shared header).
 *   Source s is VALID at a pixel when (u, v) is inside it and -- with key_plane >= 0 -- the NEAREST element of its plane key_plane
 *   differs in bits from nodata_bits[key_plane] and, with SC_MOSAIC_KEY_FLOAT (4- or 8-byte IEEE elements), is not NaN.
 *   FIRST / LAST : the valid source with the lowest / highest number wins; any element width.
 *   MAX / MIN    : float32; the valid source whose NEAREST key element is largest / smallest wins (NaN never valid; equal values go
 *                  to the lower number; the comparison is on the raw element whatever `resampling` is).  key_plane >= 0.
 *   BY_INDEX     : the winner is select[r][c] when that source is inside at the pixel (validity is not consulted); values outside
 *                  [0, N) mean none.  count must be NULL.
 *   For these five: out[p] = what sc_warp writes for plane p of the winner at its (u, v) under `resampling` (nearest: a word copy;
 *   bilinear: float32, the plane's no-data when the nearest element does not count), nodata_bits[p] without a winner; index = the
 *   winner or -1.
 *   MEAN         : float32, P <= SC_MOSAIC_MEAN_PLANES.  out[p] = the fp64 sum, in ascending source order, of the valid sources'
 *                  samples of plane p that count (nearest: the element; bilinear: the value before rounding), divided by the number
 *                  of terms and rounded once; no-data without a term.  index must be NULL.
 *   count (any rule but BY_INDEX, may be NULL) = the number of valid sources.
 * `sources` is a HOST array of N descriptors; it is checked here and copied once into `table`, device memory of at least
 * N * sizeof(sc_mosaic_source) bytes (8-byte aligned) that the kernel reads.  box = {r0, r1, c0, c1}: a half-open box of destination
 * pixels outside of which the source has no pixel (0 <= r0, r1 <= out_h, 0 <= c0, c1 <= out_w; empty allowed).  It only culls: a
 * work-group runs the per-source work for the sources whose box meets its tile, and a tile that meets none writes no-data / -1 / 0
 * before any projection; a box larger than needed changes no byte.  Planes are read in place as in sc_warp (strides in elements,
 * >= 0); nodata_bits[p] is shared by all sources.  out [P][out_h][out_w], index / count int32 [out_h][out_w].
 * CRS: every source code equals dst_crs (any code >= 0), or it and dst_crs are 4326 / WGS-84 UTM.  SC_ERR_ARG as sc_warp, and for
 * N outside [1, 64], P outside [1, 32], key_plane outside [-1, P), a rule / width combination above, a box outside the grid.
 * No LDS, no atomics: repeated calls give identical bits.                                                                       */
#define SC_MOSAIC_MAX_SOURCES 64
#define SC_MOSAIC_MEAN_PLANES 4
#define SC_MOSAIC_FIRST 0
#define SC_MOSAIC_LAST 1
#define SC_MOSAIC_MAX 2
#define SC_MOSAIC_MIN 3
#define SC_MOSAIC_MEAN 4
#define SC_MOSAIC_BY_INDEX 5
#define SC_MOSAIC_KEY_FLOAT 1 /* flags: the key plane holds IEEE floating-point numbers of elem_bytes (4 or 8); a NaN is not valid */
typedef struct sc_mosaic_source {
  double src_inv[6];                             /* world -> source pixel coordinates, as in sc_warp_args        */
  int32_t src_crs, src_h, src_w;
  int32_t reserved;                              /* 0                                                            */
  int32_t box[4];                                /* r0, r1, c0, c1 in destination pixels, half-open              */
  const void* src[SC_WARP_MAX_PLANES];           /* element (0, 0) of every plane, device                        */
  int64_t row_stride[SC_WARP_MAX_PLANES];        /* elements                                                     */
  int64_t col_stride[SC_WARP_MAX_PLANES];
} sc_mosaic_source;
typedef struct sc_mosaic_args {
  double dst_gt[6];                              /* geotransform of the destination grid, GDAL order             */
  int32_t dst_crs, out_h, out_w;
  int32_t N, P;                                  /* sources 1..64, planes per source 1..32                       */
  int32_t elem_bytes;                            /* 1, 2, 4 or 8: one width per call                             */
  int32_t rule;                                  /* SC_MOSAIC_FIRST ... SC_MOSAIC_BY_INDEX                       */
  int32_t key_plane;                             /* -1: the footprint alone decides validity                     */
  int32_t resampling;                            /* SC_WARP_NEAREST, SC_WARP_BILINEAR                            */
  int32_t flags;                                 /* SC_MOSAIC_KEY_FLOAT                                          */
  uint64_t nodata_bits[SC_WARP_MAX_PLANES];      /* raw bit pattern of every plane's no-data value               */
  const sc_mosaic_source* sources;               /* HOST, N descriptors                                          */
  void* table;                                   /* device, >= N * sizeof(sc_mosaic_source) bytes                */
  void* out;                                     /* [P][out_h][out_w] device                                     */
  int32_t* index;                                /* [out_h][out_w] device, or NULL                               */
  int32_t* count;                                /* [out_h][out_w] device, or NULL                               */
  const int32_t* select;                         /* [out_h][out_w] device: SC_MOSAIC_BY_INDEX                    */
} sc_mosaic_args;
int sc_mosaic(const sc_mosaic_args* a, sc_stream stream);

/* Cutting the sampled windows of a flight line into dense sample tensors: the reads of WindowDataset.__getitem__,
 * starcop/data/sampling_dataset.py:259-303 -- RasterioReader.read_from_window(window, boundless=True).load(boundless=True) at :266,
 * nodata -> 0 at :269-271, the acquisition-date multiply at :285 / :289 and np.clip at :287 / :293 -- for every window of a chunk
 * and every product in one launch.
 *   sc_window_cut : out[w][p][i][j], dense [n_win][P][out_h][out_w]; with (r, c) = (row_off[w] + i, col_off[w] + j)
 *                     v = plane p holds (r, c) ? src_p[(r - row0_p) * row_stride_p + (c - col0_p) * col_stride_p] : 0
 *                     if ops_p & SC_WCUT_FILL  and v == fill_p : v = 0            (a NaN fill masks nothing)
 *                     if ops_p & SC_WCUT_SCALE : v = v * scale_p                  (one float32 multiply, one rounding)
 *                     if ops_p & SC_WCUT_CLIP  : v = min(max(v, lo_p), hi_p) as numpy.clip evaluates it: NaN stays NaN
 * Reads are boundless: a window may hang over any edge of the scene, lie wholly outside it or be larger than it; offsets may be
 * negative.  Plane p is read in place through its pointer and non-negative element strides and covers rows [row0_p, row0_p + rows_p)
 * and columns [col0_p, col0_p + cols_p) of the scene (the extent must lie inside the scene_rows x scene_cols scene): a decoded
 * (H, W) plane, one band of a chunky (H, W, 4) label image (col_stride = 4), one band of a pixel-interleaved radiance cube
 * (col_stride = bands), or only the row band of a flight line that the windows touch (row0 > 0).  Nothing outside a plane's extent
 * is dereferenced.
 * One element width per call: elem_bytes 1, 2 or 4.  SC_WCUT_SCALE / SC_WCUT_CLIP need elem_bytes = 4; when any plane of the call
 * has one, every plane of the call is read as float32 and fill_p is compared as a float32 (fill_bits holds its bit pattern: -0.0
 * matches +0.0, a NaN fill matches nothing).  Without them the call is pure data movement: fill_bits is compared as a bit pattern of
 * elem_bytes and a hit is replaced by zero bits, so the result is bit-equal to the numpy restatement for every dtype of that width.
 * The float32 multiply is x * float32(s), s evaluated in float64 by the caller in the reference's order (factor / 100 /
 * solar_irradiance): what `values *= s` computes on a float32 array under numpy 1.x, the numpy of the published dataset.
 * The windows are given twice, as [n_win][2] int32 (row_off, col_off) tables on the device (for the kernel) and on the host (for the
 * checks): row_off + out_h and col_off + out_w must stay inside int32.  Every check runs on the host before the launch; the device
 * table is read back (n_win * 8 bytes) and must equal the host one, so -- the one exception to the convention above -- this call waits
 * for `stream` and cannot be captured into a graph.  1 <= P <= 64, 1 <= n_win <= 2^20, out_h * out_w < 2^31.
 * 16-byte stores when out_w * elem_bytes is a multiple of 16 and `out` is 16-byte aligned, element stores otherwise; source loads
 * assume element alignment only (col_off mod 4 takes every value).  SC_ERR_ARG for bad dims, P or n_win out of range, an
 * unsupported elem_bytes, scale / clip at 1 or 2 bytes, unordered clip bounds, null or misaligned pointers, negative strides, a
 * plane extent outside the scene, window tables that differ.  No atomics, nothing written outside `out`: repeated calls give
 * identical bits.                                                                                                              */
#define SC_WCUT_MAX_PLANES 64
#define SC_WCUT_FILL 1
#define SC_WCUT_SCALE 2
#define SC_WCUT_CLIP 4
typedef struct sc_wcut_args {
  int32_t scene_rows, scene_cols;                /* the grid the window offsets refer to                      */
  int32_t out_h, out_w;                          /* size of every window of the call                          */
  int32_t P;                                     /* planes, 1..64                                             */
  int32_t elem_bytes;                            /* 1, 2 or 4                                                 */
  int32_t n_win;
  int32_t reserved;
  const int32_t* win_off;                        /* [n_win][2] (row_off, col_off), device                     */
  const int32_t* win_off_host;                   /* the same on the host                                      */
  const void* src[SC_WCUT_MAX_PLANES];           /* element (row0, col0) of every plane, device               */
  int64_t row_stride[SC_WCUT_MAX_PLANES];        /* elements                                                  */
  int64_t col_stride[SC_WCUT_MAX_PLANES];
  int32_t row0[SC_WCUT_MAX_PLANES];              /* origin of the plane inside the scene                      */
  int32_t col0[SC_WCUT_MAX_PLANES];
  int32_t rows[SC_WCUT_MAX_PLANES];              /* its extent                                                */
  int32_t cols[SC_WCUT_MAX_PLANES];
  uint32_t ops[SC_WCUT_MAX_PLANES];              /* SC_WCUT_FILL | SC_WCUT_SCALE | SC_WCUT_CLIP               */
  uint32_t fill_bits[SC_WCUT_MAX_PLANES];        /* bit pattern of the fill value (low elem_bytes bytes)      */
  float scale[SC_WCUT_MAX_PLANES];
  float clip_lo[SC_WCUT_MAX_PLANES];
  float clip_hi[SC_WCUT_MAX_PLANES];
  void* out;                                     /* [n_win][P][out_h][out_w] device                           */
} sc_wcut_args;
int sc_window_cut(const sc_wcut_args* a, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* Whole-scene cloud masking: the reference's CDModel.predict (starcop/sentinel2/models.py:27-52, 80-89) reflect-pads the scene to a
 * multiple of 32 and runs it as ONE image; a 10 980 x 10 980 Sentinel-2 tile does not fit that way.  Here the padded scene is walked
 * in equally shaped windows (sentinel2.scene_windows); one table row describes a window to both kernels below.
 *   sc_scene_gather : out[i][c][y][x] = (float) src[c][refl(row_off_i + y - pad_top, H)][refl(col_off_i + x - pad_left, W)] [* scale]
 *                     refl(t, n) = t < 0 ? -t : (t >= n ? 2 (n - 1) - t : t): numpy's "reflect" with ONE reflection, so pads < n.
 *                     src: (C, H, W) uint16 (elem_bytes 2) or float32 (4), device, read in place through non-negative element
 *                     strides (a band-interleaved view has col_stride = C); out: dense [n][C][win_h][win_w] float32, 16-byte
 *                     aligned, win_w a multiple of 4.  scale == 1: no multiply; otherwise exactly one float32 multiply (float)v *
 *                     scale.  Addresses are 64-bit.  16-byte stores; one 8- / 16-byte load per store where its four source elements
 *                     are contiguous, inside the image and so aligned, element loads otherwise.  The padded scene is never stored.
 *   sc_head_conv_fwd_k_mosaic : the class-index path of sc_head_conv_fwd_k (logits == NULL) with a destination table: of batch item
 *                     i only the core rectangle rows [core_y0, core_y1) x columns [core_x0, core_x1) of its H x W plane is stored,
 *                     at mosaic[(dst_row + y - core_y0) * pitch + dst_col + x - core_x0].  Same stencil, same FMA order, hence the
 *                     class bits of sc_head_conv_fwd_k; work-groups whose tile holds no core pixel return before they stage
 *                     anything.  4-byte stores where four adjacent pixels are wanted and their address is 4-byte aligned, byte
 *                     stores otherwise.  An empty core (core_y1 <= core_y0 or core_x1 <= core_x0) stores nothing.
 * The table is given twice, on the device for the kernels and on the host for the checks that run before the launch (windows inside
 * the reflect-padded scene; cores inside the plane and their destinations inside the mos_h x mos_w mosaic); the kernels additionally
 * clamp source coordinates into the image and drop stores outside the mosaic, so a device table that differs from the checked one
 * cannot make them touch foreign memory.  No synchronisation, no allocation, no atomics.                                          */
typedef struct sc_scene_win {
  int32_t row_off, col_off;                      /* window origin in the padded scene (sc_scene_gather)       */
  int32_t core_y0, core_y1, core_x0, core_x1;    /* core rectangle inside the window (mosaic head)            */
  int32_t dst_row, dst_col;                      /* where the core's first pixel goes in the mosaic           */
} sc_scene_win;
typedef struct sc_scene_args {
  const void* src;                               /* element [0][0][0], device                                 */
  int32_t elem_bytes;                            /* 2 = uint16, 4 = float32                                   */
  int32_t C, H, W;
  int64_t chan_stride, row_stride, col_stride;   /* elements                                                  */
  int32_t pad_top, pad_left;                     /* reflect pads in front of row 0 / column 0                 */
  int32_t n, win_h, win_w;                       /* windows of the call and their common shape                */
  float scale;
  const sc_scene_win* win;                       /* [n] device                                                */
  const sc_scene_win* win_host;                  /* the same on the host                                      */
  float* out;                                    /* [n][C][win_h][win_w] device                               */
} sc_scene_args;
int sc_scene_gather(const sc_scene_args* a, sc_stream stream);
int sc_head_conv_fwd_k_mosaic(const sc_src* in, const float* w /*[K][Cin][3][3]*/, const float* bias /*[K]*/,
                              uint8_t* mosaic /*[mos_h][pitch]*/, int mos_h, int mos_w, int64_t pitch,
                              const sc_scene_win* win /*[N] device*/, const sc_scene_win* win_host /*[N] host*/,
                              int N, int Cin, int K, int H, int W, sc_stream stream);

/* Whole flight lines through the binary plume model (ModelModule.predict_scene): the same window table, three more entry points.
 *   sc_scene_gather_planes : sc_scene_gather for 1 <= P <= SC_SCENE_MAX_PLANES float32 planes that each have their own base pointer
 *                     and non-negative element strides (three bands of one (H, W, 3) buffer are three planes with column stride 3),
 *                     with the per-plane operation of sc_window_cut applied to every element in sc_window_cut's order:
 *                       ops_p & SC_WCUT_FILL and the element's BIT PATTERN == fill_bits_p : 0.0f
 *                       else if ops_p & SC_WCUT_SCALE : v * scale_p                  (one float32 multiply, one rounding)
 *                       then if ops_p & SC_WCUT_CLIP  : v < lo ? lo : v, then v > hi ? hi : v   (numpy.clip: NaN stays NaN)
 *                     (the fill is compared as bits here -- -0.0 does not match +0.0, a NaN pattern matches itself -- so that it is
 *                     the test sc_scene_core_counts and the mosaic head make.)  out: dense [n][P][win_h][win_w] float32, 16-byte
 *                     aligned, win_w a multiple of 4; 16-byte stores; one 16-byte load per store where its four sources are
 *                     contiguous, inside the image and so aligned, element loads otherwise.  A plane with ops == 0 passes its bits
 *                     through: what sc_scene_gather (scale 1) gives for the same plane.
 *   sc_scene_core_counts : counts[i] (int32) = number of pixels of window i's core DESTINATION rectangle -- rows dst_row .. dst_row +
 *                     core_y1 - core_y0, columns likewise -- of one float32 plane whose bits differ from fill_bits; 0 for an empty
 *                     core.  counts is overwritten.  Integer sums (one integer atomic per work-group): the result does not depend
 *                     on the launch geometry.  A core may hold at most 2^31 - 1 pixels.
 *   sc_head_conv_fwd_mosaic_prob : the 1-class head (sc_head_conv_fwd: Cin <= 32, RAW / AFFINE, no upsample) with the destination
 *                     table of sc_head_conv_fwd_k_mosaic.  Per core pixel z = the logit of sc_head_conv_fwd (same stencil and FMA
 *                     order, hence its bits whichever of its kernels the shape selects), p = 1.f / (1.f + expf(-z)), m = p > 0.5f
 *                     (sc_threshold_masks with ge0 = 0); p goes to the float32 mosaic `prob` (pitch in elements), m to the uint8
 *                     mosaic `mask`; either may be NULL, not both.  valid != NULL: a float32 plane addressed like the mosaics
 *                     (valid[r * valid_row_stride + c * valid_col_stride] for mosaic pixel (r, c)); where its bits equal fill_bits
 *                     the pixel gets `nodata` and 0 instead.  Logits are never stored; tiles without a core pixel leave before
 *                     they stage anything; 16- / 4-byte stores where four adjacent pixels are wanted and aligned, element stores
 *                     otherwise.
 * Checks and guarantees are those of the two functions above: everything is validated on the host copy of the table before a launch
 * (SC_ERR_ARG otherwise), the kernels clamp reads into the planes and drop stores outside the mosaics / the image whatever the
 * device table holds.  No allocation, no synchronisation, no floating-point atomics, 64-bit addresses.                           */
#define SC_SCENE_MAX_PLANES 16
typedef struct sc_scene_planes_args {
  int32_t P, H, W;                               /* planes (1..16) and their common size                      */
  int32_t pad_top, pad_left;                     /* reflect pads in front of row 0 / column 0                 */
  int32_t n, win_h, win_w;                       /* windows of the call and their common shape                */
  const float* src[SC_SCENE_MAX_PLANES];         /* element [0][0] of every plane, device                     */
  int64_t row_stride[SC_SCENE_MAX_PLANES];       /* elements                                                  */
  int64_t col_stride[SC_SCENE_MAX_PLANES];
  uint32_t ops[SC_SCENE_MAX_PLANES];             /* SC_WCUT_FILL | SC_WCUT_SCALE | SC_WCUT_CLIP               */
  uint32_t fill_bits[SC_SCENE_MAX_PLANES];       /* bit pattern of the fill value                             */
  float scale[SC_SCENE_MAX_PLANES];
  float clip_lo[SC_SCENE_MAX_PLANES];
  float clip_hi[SC_SCENE_MAX_PLANES];
  const sc_scene_win* win;                       /* [n] device                                                */
  const sc_scene_win* win_host;                  /* the same on the host                                      */
  float* out;                                    /* [n][P][win_h][win_w] device                               */
} sc_scene_planes_args;
int sc_scene_gather_planes(const sc_scene_planes_args* a, sc_stream stream);
int sc_scene_core_counts(const float* plane, int64_t row_stride, int64_t col_stride, int H, int W, uint32_t fill_bits,
                         const sc_scene_win* win /*[n] device*/, const sc_scene_win* win_host /*[n] host*/, int n,
                         int32_t* counts /*[n] device*/, sc_stream stream);
int sc_head_conv_fwd_mosaic_prob(const sc_src* in, const float* w /*[1][Cin][3][3]*/, const float* bias /*[1]*/,
                                 float* prob /*[mos_h][prob_pitch] or NULL*/, int64_t prob_pitch,
                                 uint8_t* mask /*[mos_h][mask_pitch] or NULL*/, int64_t mask_pitch, int mos_h, int mos_w,
                                 const float* valid /*or NULL*/, int64_t valid_row_stride, int64_t valid_col_stride,
                                 uint32_t fill_bits, float nodata,
                                 const sc_scene_win* win /*[N] device*/, const sc_scene_win* win_host /*[N] host*/,
                                 int N, int Cin, int H, int W, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* evaluation masks of the baselines and of run_validation.
 * Thresholded prediction with an optional binary opening by a 3x3 structuring element:
 *   starcop/baselines.py:25-27 binary_opening = dilation(erosion(x)) ; :53-57 Mag1cBaseline.apply_threshold (pred > thr, cross SE)
 * kornia.morphology.{erosion,dilation} (third-party, absent from /root/reference: restated from its published algorithm,
 * border_type='geodesic', engine='unfold'): erosion = min over the SE's set cells, pixels outside the image never lower the
 * minimum; dilation = max over the cells of the SE flipped in both axes, pixels outside never raise the maximum.
 * se_bits: bit (3*r + c) set <=> SE[r][c] != 0; 0 = no morphology (plain pred > thr); the cross of the reference is 0xBA.
 *   sc_binary_opening      : out[n][h][w] (int64) = opening(pred > thr); tile_count[n] += sum(out[n]) if not NULL
 *   sc_threshold_confusion : for T <= 32 thresholds at once (validation.py:38,121-127: the PR curve; T = 1: the per-tile
 *                            matrix :106) cm[n][t][2*target + p] += 1, p = the mask above at thresholds[t] (host array),
 *                            target = (int64)target_f32 in {0, 1} (other values are counted in *invalid and skipped);
 *                            pixels with ignore[i] != 0 are skipped (validation.py:84-100 mask_from_magic).            */
#define SC_SE_CROSS 0xBA
int sc_binary_opening(const float* pred, float threshold, int se_bits, int64_t* out, int64_t* tile_count,
                      int N, int H, int W, sc_stream stream);
int sc_threshold_confusion(const float* pred, const float* target, const unsigned char* ignore,
                           const float* thresholds, int T, int se_bits, int64_t* cm, int64_t* invalid,
                           int N, int H, int W, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* training-batch assembly from tiles resident in HBM: crop a window of a stored tile and apply the
 * spatial augmentations of starcop/data/datamodule.py:128-134 (kornia 0.6.7 RandomRotation(degrees=90, p=.5) ->
 * RandomHorizontalFlip(p=.5) -> RandomVerticalFlip(p=.5), applied in that order by starcop/data/dataset.py:99-102) in one
 * gather: out[b][c][y][x] = crop_b(ys, xs) with (x, y) un-flipped, then rotated about the crop centre ((w-1)/2, (h-1)/2):
 *   xs = cx + cos*(x - cx) - sin*(y - cy),  ys = cy + sin*(x - cx) + cos*(y - cy)
 * sampled bilinearly (mode 0) or at the nearest pixel (mode 1) with zeros outside the crop -- what kornia's rotate() ->
 * warp_affine -> F.grid_sample(align_corners=True, padding_mode="zeros") computes.  Items without the rotate flag are
 * exact copies.  Per-item arrays are device pointers: tile index, window offsets, cos/sin, flags (1 rotate, 2 hflip,
 * 4 vflip).  tiles: [M][C][Hs][Ws] f32, out: [B][C][h][w] f32.                                                       */
int sc_gather_augment(const float* tiles, int M, int C, int Hs, int Ws, const int32_t* tile, const int32_t* row_off,
                      const int32_t* col_off, const float* cos_t, const float* sin_t, const int32_t* flags, int B,
                      int h, int w, int mode, float* out, sc_stream stream);

/* Label sums of the training windows of the resident tiles (starcop/data/datamodule.py:17-64, tiled_dataframe: frac_positives =
 * torch.sum(label window) / window size):  out[m][k] = sum of labels[m][r][c] over window k = (row_off, col_off, height, width),
 * accumulated in fp64.  labels: [M][H][W] f32 dense, device; the K windows are shared by all tiles and given twice, on the device
 * for the kernel and on the host for the argument check that runs before the launch; out: [M][K] f64 device.  Any H, W >= 1 with
 * H*W < 2^31 and any window inside the tile (width 1, odd offsets, overlapping, repeated, the whole tile).  One launch, no
 * workspace, no allocation, no synchronisation.  The additions have a fixed order (per-lane fp64 partials, wavefront shuffle, LDS)
 * and there are no atomics: repeated calls give identical bits, and windows whose partial sums are integers below 2^53 ({0, 1}
 * labels) are exact.  16-byte loads where a row segment is 16-byte aligned, element loads at its ragged ends.  SC_ERR_ARG for
 * M < 1, K < 1, bad dims, a null or misaligned pointer, an empty window or one that leaves the tile; nothing is launched then.  */
int sc_tile_window_sums(const float* labels, int M, int H, int W, const int32_t* windows, const int32_t* windows_host, int K,
                        double* out, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* Regression path (starcop/models/model_module_regression.py): the pointwise networks SimpleCNN_v2 (one 1x1 convolution) and
 * SimpleCNN_v3 (two, no activation between them; models/architectures/baselines.py:43-70) and the losses of
 * models/utils/losses.py (F.l1_loss / F.mse_loss, default reduction).
 *
 * Network: Cin -> C1 [-> Cout], every count in 1..SC_PWREG_MAXC, `layers` 1 or 2 (one layer: C1 == Cout), bias always present.
 * `params` is one flat fp32 device buffer in state_dict order: W1[C1][Cin], b1[C1], then for two layers W2[Cout][C1], b2[Cout]
 * (sc_pwreg_param_floats of them; 0 for an unsupported shape).  Tensors are dense NCHW fp32, any H*W >= 1.
 *
 *   sc_pwreg_fwd          pred[N][Cout][H][W] from x[N][Cin][H][W], layer by layer in fp32 (an fmaf chain over ascending input
 *                         channel, starting from the bias).  16-byte loads and stores when H*W is a multiple of 4 and both
 *                         tensors start on 16-byte boundaries (then every plane does), element accesses otherwise.
 *   sc_reg_loss           *loss_sum = sum |pred - y| (SC_REG_L1) or sum (pred - y)^2 (SC_REG_MSE) over n elements, in fp64 (the
 *                         caller divides by n); dpred (optional) = d mean / d pred = sign(pred - y) / n with sign(0) = 0, or
 *                         2 (pred - y) / n.  work: SC_REG_LOSS_PARTS doubles.  Fixed summation order, no atomics.
 *   sc_pwreg_train_sweep  one pass over x and y: prediction and g = sign(pred - y) | (pred - y) in registers, nothing of that
 *                         size is stored; mode SC_PWREG_G_FROM_MEMORY reads g[N][Cout][H][W] from y_or_g instead (params may be
 *                         NULL).  Writes sc_pwreg_sweep_blocks(N, H, W) partial rows of SC_PWREG_PART_DOUBLES doubles:
 *                         M[16][16] = sum_pixels g x^T, s[16] = sum_pixels g, and the loss sum.
 *   sc_pwreg_finalize     one work-group: sums the rows in a fixed order, multiplies the moments by `scale` (1/n for L1, 2/n for
 *                         MSE, 1 for g from memory), forms in fp64   one layer: dW = M, db = s;   two layers: dW2 = M W1^T + s b1^T,
 *                         db2 = s, dW1 = W2^T M, db1 = W2^T s   and writes grad (fp32, flat, parameter order) and, if not NULL,
 *                         *loss_sum (unscaled).
 * No floating-point atomics anywhere; the sweep's grid depends on N*H*W only; equal inputs give equal bits.                  */
#define SC_PWREG_MAXC 16
#define SC_PWREG_PART_DOUBLES 273
#define SC_REG_LOSS_PARTS 256
enum sc_reg_loss_kind { SC_REG_L1 = 0, SC_REG_MSE = 1, SC_PWREG_G_FROM_MEMORY = 2 };
size_t sc_pwreg_param_floats(int Cin, int C1, int Cout, int layers);
int sc_pwreg_fwd(const float* x, const float* params, int N, int Cin, int C1, int Cout, int layers, int H, int W, float* pred,
                 sc_stream stream);
int sc_reg_loss(const float* pred, const float* y, size_t n, int kind, double* loss_sum, float* dpred, double* work,
                sc_stream stream);
int sc_pwreg_sweep_blocks(int N, int H, int W);
int sc_pwreg_train_sweep(const float* x, const float* y_or_g, const float* params, int N, int Cin, int C1, int Cout, int layers,
                         int H, int W, int mode, double* part, sc_stream stream);
int sc_pwreg_finalize(const double* part, int nblocks, const float* params, int Cin, int C1, int Cout, int layers, double scale,
                      float* grad, double* loss_sum, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* Validation panels (starcop/plot.py plot_batch, starcop/validation.py:137-153): a figure is a canvas of image panels, each one a
 * source plane (or three) of a batch tensor turned into 8-bit RGB and enlarged by an integer nearest-neighbour factor.  The canvas is
 * stored as PNG scanlines: canvas_h rows of 1 + 3 * canvas_w bytes, byte 0 of a row is the filter byte 0, RGB triplets follow, so the
 * buffer goes to zlib as it is.  Every byte of the canvas is written: pixels outside every panel are white (255).
 *
 * Per pixel, all arithmetic in float32 (DESIGN.md "Validation panels" has the derivation from matplotlib):
 *   SC_PANEL_BAND         v = (float)src; if div != 1: v = v / div.  Not finite -> white.  Else t = (v - vmin) / d with
 *                         d = (float)((double)vmax - (double)vmin), t = 0 if vmax == vmin; xa = t * 256f; index = 0 if xa < 0,
 *                         255 if xa >= 256, else trunc(xa); colour = viridis[index] (256 x 3 bytes, starcop_amd/data/viridis8.txt).
 *   SC_PANEL_RGB          per channel c = min(max(v, 0), 1), byte = trunc(c * 255f); a NaN in any channel -> white.
 *   SC_PANEL_CATEGORICAL  the colour of the LAST of the n_cat entries whose value equals (float)src; no match -> (0, 0, 0).
 *
 *   sc_panel_minmax   out[p] = (min, max) over the finite v of panel p's plane when it is flagged autoscale, (0, 1) if it has none;
 *                     (vmin, vmax) of the descriptor otherwise, so out holds the range every panel is drawn with.  One launch, one
 *                     work-group per panel, min/max only (no sums): equal inputs give equal bits.
 *   sc_render_panels  one launch for the whole figure; an autoscale panel takes its range from minmax[p] (may be NULL when no
 *                     panel is flagged), which the preceding sc_panel_minmax on the same stream left there -- no host
 *                     synchronisation in between.
 * The table is given twice (as for sc_scene_gather): on the device for the kernel, on the host for the checks made before the
 * launch.  SC_ERR_ARG, with nothing launched, for n_panels outside [1, SC_PANEL_MAX], a null pointer, an unknown dtype or kind,
 * scale < 1, bad dims or stride, autoscale on a panel that is not a BAND, a div that is 0 or not finite, limits that are not
 * finite, n_cat outside [0, SC_PANEL_MAX_CAT], a destination rectangle that leaves the canvas, or two rectangles that overlap. */
#define SC_PANEL_MAX 1024
#define SC_PANEL_MAX_CAT 8
enum sc_panel_dtype { SC_PANEL_F32 = 0, SC_PANEL_I64 = 1, SC_PANEL_U8 = 2 };
enum sc_panel_kind { SC_PANEL_BAND = 0, SC_PANEL_RGB = 1, SC_PANEL_CATEGORICAL = 2 };
typedef struct sc_panel {
  const void* src[3];                            /* device planes: one (BAND, CATEGORICAL) or three (RGB: r, g, b)  */
  int64_t row_stride;                            /* elements between rows of a plane (>= W)                         */
  int32_t dtype, kind;                           /* enum sc_panel_dtype, enum sc_panel_kind                         */
  int32_t H, W, scale;                           /* source size; the panel covers H*scale x W*scale canvas pixels   */
  int32_t dst_y, dst_x;                          /* its top-left canvas pixel                                       */
  int32_t autoscale, n_cat, reserved;
  float vmin, vmax, div;                         /* BAND limits (ignored when autoscale) and divisor (1 = none)     */
  float cat_value[SC_PANEL_MAX_CAT];
  uint8_t cat_rgb[SC_PANEL_MAX_CAT][4];          /* r, g, b, unused                                                 */
} sc_panel;
int sc_panel_minmax(const sc_panel* table_dev, const sc_panel* table_host, int n_panels, float* out_minmax_dev /*[n][2]*/,
                    sc_stream stream);
int sc_render_panels(const sc_panel* table_dev, const sc_panel* table_host, int n_panels, const float* minmax_dev /*[n][2]*/,
                     uint8_t* canvas, int canvas_h, int canvas_w, sc_stream stream);

/* Per-component statistics of a label image: the plume catalogue (starcop_amd/plumes.py).  Component k of image n is the set of
 * pixels of labels[n] with value k, 1 <= k <= min(counts[n], M); 0 is background.  Nothing assumes that a value is connected or
 * that the image comes from sc_connected_components, and values outside [0, min(counts[n], M)] are ignored and never index
 * memory.  counts is a DEVICE array; M is the row capacity per image the caller chose (>= the largest count it wants reported).
 * Row n*M + k-1 of every per-component column, and entry (n*M + k-1)*P + q of every per-plane column, receive:
 *   area (int64)   row_min row_max col_min col_max (int32, inclusive)   sum_row sum_col (int64)
 *   first_pixel (int64, the smallest raster index r*W + c)   n_other (int64, pixels with other != 0; 0 without `other`)
 *   per plane q < P, over the FINITE values of the component only: n_finite (int64), sum (fp64), max, min (float32), argmax
 *   (int64, the smallest raster index whose value compares equal to max); with no finite value: 0, 0, NaN, NaN, -1.
 * A value in [1, counts[n]] that no pixel carries gives area 0, a zero box, first_pixel -1 and the "no finite value" plane
 * entries.  Rows at or above counts[n] are zero-filled in every column.
 * Plane q of image n is the dense H x W float32 block at plane[q] + n*plane_stride[q] (elements), `other` likewise in bytes:
 * channel c of an (N, C, H, W) tensor is read in place.  N <= 65535, H*W < 2^31, 0 <= P <= SC_CSTATS_MAX_PLANES, M >= 0 (M = 0:
 * nothing to write, nothing launched); SC_ERR_ARG, before any launch, for bad dims, a null pointer, a plane stride below H*W in
 * a batch or a workspace that is too small.
 * Integer atomics for the bounding boxes only; the fp64 sums are added in an order that depends on the label image alone (per
 * lane in raster order along the component's box, one fixed butterfly, then the row bands of the box in order), so repeated
 * calls give identical bits and an image gives the same bits alone and inside any batch.  5 launches per call; the work is
 * proportional to the sum of the areas of the bounding boxes.
 * work: sc_component_stats_workspace_bytes(N, H, W, M, P) bytes (4 bytes and, at P planes, 40 + 32 P bytes per row, the latter
 * also per 4096 pixels of an image).                                                                                          */
#define SC_CSTATS_MAX_PLANES 8
typedef struct sc_cstats_args {
  const int32_t* labels;                          /* [N][H][W] device                                              */
  const int32_t* counts;                          /* [N] device                                                    */
  int32_t N, H, W, M, P, reserved;
  const float* plane[SC_CSTATS_MAX_PLANES];       /* element (0, 0) of image 0 of every plane                      */
  int64_t plane_stride[SC_CSTATS_MAX_PLANES];     /* elements between images                                       */
  const uint8_t* other;                           /* may be NULL                                                   */
  int64_t other_stride;                           /* bytes between images                                          */
  int64_t* area;                                  /* [N][M] columns ...                                            */
  int32_t *row_min, *row_max, *col_min, *col_max;
  int64_t *sum_row, *sum_col, *first_pixel, *n_other;
  int64_t* n_finite;                              /* [N][M][P] columns (may be NULL when P = 0) ...                */
  double* sum;
  float *max, *min;
  int64_t* argmax;
} sc_cstats_args;
size_t sc_component_stats_workspace_bytes(int N, int H, int W, int M, int P);
int sc_component_stats(const sc_cstats_args* a, void* work, size_t work_bytes, sc_stream stream);

/* Radial profiles per component: the integrated enhancement inside circles around an origin, the plume's extent and its second
 * moments (starcop_amd/plumes.py: component_radial; starcop_amd/quantify.py turns them into emission rates).  labels, counts, M and
 * the rows are those of sc_component_stats; row_min .. col_max are the box columns that call returned (inclusive; they are cut
 * to the image before they are walked, so a wrong box gives other numbers and never another address).  origin[(n*M + k-1)*2 + {0,
 * 1}] is the (row, column) the distances of component k are taken from, anywhere within +-2^30; a negative row skips the plume.
 * For every pixel (r, c) of value k inside its box, d2 = (r - r0)^2 + (c - c0)^2 in integers.  edge2[0 .. K-1], 0 <= edge2[0],
 * strictly increasing, are the squared bin edges: bin j is the smallest j with d2 <= edge2[j], bin K holds what lies beyond.
 * Per row:  bin_count (int64) and bin_sum (fp64), [K+1] each, over the pixels whose plane value is FINITE;
 *   d2_max (int64, over all pixels of the component, finite or not; -1 for a row without pixels or a skipped one);
 *   sum_rr sum_cc sum_rc (int64: the sums of r^2, c^2 and r c of the pixel indices over all pixels; with H, W <= 32767 and
 *   H*W < 2^31 they stay below 2^62).
 * Rows at or above counts[n], rows without pixels and skipped rows are zero with d2_max = -1.
 * The plane of image n is the dense H x W float32 block at plane + n*plane_stride (elements).  N <= 65535, H, W <=
 * SC_CRADIAL_MAX_SIDE, H*W < 2^31, 1 <= K <= SC_CRADIAL_MAX_BINS, M >= 0 (M = 0: nothing launched); SC_ERR_ARG, before any
 * launch, for bad dims, K out of range, edges that do not increase, a null pointer, a plane stride below H*W in a batch or a
 * workspace that is too small.
 * No floating-point atomics.  One wave walks a row band of a box in raster order, 64 pixels a step; per step and per distinct bin
 * one fixed butterfly sums the values of the lanes in that bin, the bins of a step in the order of their first lane, and the
 * bands are folded in order: the order of every fp64 addition is fixed by the label image, the boxes, the origins and the edges,
 * so repeated calls give identical bits and an image gives the same bits alone and inside any batch.  3 launches per call.
 * work: sc_component_radial_workspace_bytes(N, H, W, M, K) bytes (4 bytes and 32 + 16 (K+1) bytes per row, the latter also per
 * 512 pixels of an image).                                                                                                   */
#define SC_CRADIAL_MAX_BINS 64
#define SC_CRADIAL_MAX_SIDE 32767
typedef struct sc_cradial_args {
  const int32_t* labels;                          /* [N][H][W] device                                              */
  const int32_t* counts;                          /* [N] device                                                    */
  int32_t N, H, W, M, K, reserved;
  const int32_t *row_min, *row_max, *col_min, *col_max;   /* [N][M] device: the boxes of sc_component_stats        */
  const int32_t* origin;                          /* [N][M][2] device: (row, column); row < 0 skips the plume      */
  const float* plane;                             /* element (0, 0) of image 0                                     */
  int64_t plane_stride;                           /* elements between images                                       */
  int32_t edge2[SC_CRADIAL_MAX_BINS];             /* host values: the squared bin edges, K of them                 */
  int64_t* bin_count;                             /* [N][M][K+1] columns ...                                       */
  double* bin_sum;
  int64_t *d2_max, *sum_rr, *sum_cc, *sum_rc;     /* [N][M] columns                                                */
} sc_cradial_args;
size_t sc_component_radial_workspace_bytes(int N, int H, int W, int M, int K);
int sc_component_radial(const sc_cradial_args* a, void* work, size_t work_bytes, sc_stream stream);

/* Exact order statistics per component: the ring median, the MAD and the percentiles of a plume's own pixels
 * (starcop_amd/plumes.py: component_quantiles, component_median_mad).  labels, counts, M and the rows are those of
 * sc_component_stats: component k of image n is the set of pixels of labels[n] with value k, 1 <= k <= min(counts[n], M), connected
 * or not (a ring label image is an ordinary input); values outside that range are ignored and never index memory.
 * The plane of image n is the dense H x W float32 block at plane + n*plane_stride (elements), read in place.  The value of a pixel
 * is t = v without `center`, and t = |v - center[n*M + k-1]| with it (device float32 [N][M]; the subtraction rounded once to
 * float32).  The MEMBERS of a component are its pixels with finite t: NaN and +-inf are dropped, and so is every pixel of a row
 * whose centre is not finite.
 * Per row n*M + k-1:  n_finite (int64) the number of members;  quantile[(n*M + k-1)*Q + j] (float32) order statistic j of them.
 * No member, or a row at or above counts[n]: n_finite 0 and NaN quantiles.
 * q[j], j < Q (1 <= Q <= SC_CQUANT_MAX_Q), is the fraction float32(percent) / float32(100) in [0, 1], a negative entry asks for
 * the median.  With n members sorted ascending as s (the rule of sc_window_stats: what numpy >= 2.0 evaluates for float32 data):
 *   percentile: vi = float32(n - 1) * q[j], lo = min(floor(vi), n-1), hi = min(lo+1, n-1), g = vi - floor(vi) (0 when n = 1),
 *               d = s[hi] - s[lo], result s[lo] + d * g, or s[hi] - d * (1 - g) where g >= 0.5;
 *   median:     (s[(n-1)/2] + s[n/2]) / 2;
 * every operation rounded to float32, none fused.  The sign of a zero result is unspecified (-0.0 and +0.0 are equal values).
 * Keys are the monotone map of the float bits (sign bit flipped for non-negatives, all bits inverted for negatives), so values of
 * both signs are ordered.  Members are counted per row, every row takes a contiguous segment of a key buffer, the keys are
 * scattered into the segments, and then a segment of at most 64 keys is sorted by one wave, one of at most SC_CQUANT_SMALL_MAX keys
 * in LDS by one work-group, and the larger ones go through a four-pass 8-bit radix select over their contiguous keys, all 2 Q
 * ranks of a segment together.
 * Integer atomics only (counters, slots, histograms), no floating-point atomics, and the selection is exact: repeated calls give
 * identical bytes and an image gives the same bytes alone and inside any batch.  13 launches and one clear per call (5 when no
 * image can hold a segment above SC_CQUANT_SMALL_MAX).
 * N <= 65535, H*W < 2^31, N*H*W < 2^32, N*M < 2^31, M >= 0 (M = 0: nothing launched); SC_ERR_ARG, before any launch, for bad dims,
 * Q out of range, a q entry above 1 or NaN, a null pointer, a plane stride below H*W in a batch or a workspace that is too small.
 * work: sc_component_quantiles_workspace_bytes(N, H, W, M, Q) bytes: with L = min(N*M, N*H*W / (SC_CQUANT_SMALL_MAX + 1)) the most
 * large segments the images can hold, 4 bytes per pixel (keys) + 12 bytes per row (count, slot cursor, segment start) +
 * L * (1 KiB + 16 KiB histograms + 272 bytes of state) + 8 bytes * (N*H*W / 4096 + L) work items, each part rounded up to 256
 * bytes, + 256: about 8 bytes per pixel and 12 per row.                                                                        */
#define SC_CQUANT_MAX_Q 8
#define SC_CQUANT_SMALL_MAX 4096
typedef struct sc_cquant_args {
  const int32_t* labels;                          /* [N][H][W] device                                              */
  const int32_t* counts;                          /* [N] device                                                    */
  int32_t N, H, W, M, Q, reserved;
  const float* plane;                             /* element (0, 0) of image 0                                     */
  int64_t plane_stride;                           /* elements between images                                       */
  const float* center;                            /* [N][M] device, or NULL                                        */
  float q[SC_CQUANT_MAX_Q];                       /* host values: fractions in [0, 1]; negative = median           */
  int64_t* n_finite;                              /* [N][M] device                                                 */
  float* quantile;                                /* [N][M][Q] device                                              */
} sc_cquant_args;
size_t sc_component_quantiles_workspace_bytes(int N, int H, int W, int M, int Q);
int sc_component_quantiles(const sc_cquant_args* a, void* work, size_t work_bytes, sc_stream stream);

/* Outlines of the components of a label image: polygon rings per plume (starcop_amd/plumes.py: component_outlines).  labels is
 * one int32 H x W image, 0 (and anything below) background, component k the pixels of value k.  The outline of k is made of
 * directed unit edges on the (H+1) x (W+1) lattice of pixel corners (corner (r, c) = the upper-left corner of pixel (r, c)),
 * one for every side of a pixel of value k whose neighbour is not k or lies outside, directed so that k is on the RIGHT (row axis
 * down): top (r,c)->(r,c+1), right (r,c+1)->(r+1,c+1), bottom (r+1,c+1)->(r+1,c), left (r+1,c)->(r,c).  Edges are numbered in
 * raster order of their pixel, then top, right, bottom, left.  The successor of an edge is the edge of the same value that leaves
 * its end corner; where two pixels of k meet diagonally with neither of the other two being k, connectivity 2 turns left (crosses
 * to the diagonal pixel), connectivity 1 turns right.  The cycles of the successor are the rings; a ring's signed doubled area is
 * sum(col_i * row_{i+1} - col_{i+1} * row_i): > 0 an exterior, < 0 a hole.  A ring may touch itself at such a corner.
 * The call is made in stages, the caller's scans and sort between them (all buffers device memory, one stream):
 *   SC_OUTLINE_COUNT   cnt[H*W] <- boundary sides per pixel.       caller: prefix = inclusive scan of cnt, E = prefix[H*W-1]
 *   SC_OUTLINE_TRACE   successors, ceil(log2 E) + 1 pointer-doubling launches, areas.  keys[E] <- (value << 33 | hole << 32 | the
 *                      ring's smallest edge) at that edge, INT64_MAX elsewhere; stats[2] <- {rings R, corner vertices}
 *                                                                  caller: sorted_keys = the R smallest keys in ascending order
 *   SC_OUTLINE_RINGS   ring_label[R], ring_area2[R], ring_len[R] (edges of the ring) in that order: value, exterior first, first
 *                      edge.                                       caller: ring_start[R+1] = exclusive scan of ring_len
 *   SC_OUTLINE_SCATTER ordered[E][2] <- (row, col) of the start corner of every edge, ring after ring, each from its smallest
 *                      edge on; ordered_keep[E] <- 1 where the incoming and the outgoing edge differ in direction.
 *                                                                  caller: keep_prefix = inclusive scan of ordered_keep
 *   SC_OUTLINE_COMPACT vertices[V][2] <- the kept corners; ring_offsets[R+1] <- their ring boundaries (V = stats[1]).
 * With every vertex wanted, `ordered` and `ring_start` are the result and COMPACT is not called.  E = 0 needs no call after COUNT.
 * work: sc_component_outlines_workspace_bytes(H, W, E) bytes, the same buffer from TRACE to the last stage; cnt and prefix are
 * the only per-pixel buffers (8 bytes per pixel).  SC_ERR_ARG, before any launch, when 4*H*W >= 2^31 (the workspace size is then
 * 0), for a connectivity other than 1 or 2, a null pointer the stage needs, counts out of range or a workspace that is too
 * small.  Integer arithmetic and integer atomic adds only: repeated calls give identical bytes.  No launch waits on another
 * work-group: every doubling round is its own launch.                                                                       */
enum sc_outline_stage { SC_OUTLINE_COUNT = 0, SC_OUTLINE_TRACE = 1, SC_OUTLINE_RINGS = 2, SC_OUTLINE_SCATTER = 3, SC_OUTLINE_COMPACT = 4 };
typedef struct sc_outline_args {
  const int32_t* labels;                          /* [H][W]                                                        */
  int32_t H, W, connectivity, reserved;
  int64_t E, R, V;                                /* edges (from TRACE on), rings (from RINGS on), vertices (COMPACT) */
  int32_t* cnt;                                   /* [H*W]                                                         */
  const int32_t* prefix;                          /* [H*W] inclusive scan of cnt                                   */
  void* work;
  size_t work_bytes;
  int64_t* keys;                                  /* [E]                                                           */
  int32_t* stats;                                 /* [2]                                                           */
  const int64_t* sorted_keys;                     /* [R]                                                           */
  int32_t* ring_label;                            /* [R]                                                           */
  int64_t* ring_area2;                            /* [R]                                                           */
  int64_t* ring_len;                              /* [R]                                                           */
  const int64_t* ring_start;                      /* [R+1]                                                         */
  int32_t* ordered;                               /* [E][2]                                                        */
  int32_t* ordered_keep;                          /* [E]                                                           */
  const int32_t* keep_prefix;                     /* [E] inclusive scan of ordered_keep                            */
  int32_t* vertices;                              /* [V][2]                                                        */
  int64_t* ring_offsets;                          /* [R+1]                                                         */
} sc_outline_args;
size_t sc_component_outlines_workspace_bytes(int H, int W, int64_t E);
int sc_component_outlines_rounds(int64_t E);      /* pointer-doubling launches of TRACE for E edges                 */
int sc_component_outlines(const sc_outline_args* a, int stage, sc_stream stream);

/* Polygons -> label image: the inverse of sc_component_outlines (starcop_amd/plumes.py: rasterize_polygons).  P polygons, each a
 * set of rings given as directed edges (x0, y0) -> (x1, y1) in PIXEL coordinates, float64, x along the columns and y along the
 * rows: pixel (r, c) covers [c, c+1) x [r, r+1), its centre is (c + 0.5, r + 0.5).  The caller closes every ring (the closing
 * edge is in the list); winding is irrelevant.  out is one int32 H x W image, 0 where no polygon covers the pixel.
 *   coverage   even-odd over ALL edges of a polygon: exteriors, holes, the parts of a multi-polygon and rings that touch
 *              themselves need no distinction.
 *   crossing   an edge crosses the scanline of row r, yc = r + 0.5 (exact in float64), iff (y0 <= yc) != (y1 <= yc): horizontal
 *              edges never cross, a vertex on a scanline counts once.
 *   abscissa   xs = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0) in float64, every operation rounded on its own -- subtract,
 *              multiply, divide, add -- with no fused multiply-add (the file is compiled with contraction off).
 *   toggle     the crossing toggles pixel c of row r iff xs <= c + 0.5; a pixel is covered when its toggle count is odd.  A
 *              top-left rule: the square (2.5, 2.5) .. (6.5, 6.5) covers rows 2..5 and columns 2..5, not 6.  Away from ties this
 *              is GDAL's default burn (pixel centre inside, no ALL_TOUCHED).
 *   order      polygon i (0-based) burns i + 1; where polygons overlap the one later in the list wins (integer atomicMax of
 *              i + 1: independent of scheduling, two calls give identical bytes).  With values != NULL a second launch maps
 *              i + 1 -> values[i] in place (any int32, repeats allowed); NULL leaves 1..P.
 *   clipping   vertices may lie anywhere (|coordinate| < 2^31, finite: the caller checks); each polygon carries a box of rows
 *              [r0, r1) and columns [c0, c1) inside the raster that contains every pixel it can toggle, one column to spare for
 *              the rounding of xs.  A crossing left of the box toggles the whole box row, one right of it nothing.
 * The polygon table is given twice (as for sc_scene_gather): on the device for the kernel, on the host for the checks made before
 * the launch.  job0 is the running sum of the rows r1 - r0 of the polygons before it that have a non-empty box and at least one
 * edge: one wave per (polygon, row).  There is no cap on crossings per row, edges per polygon or polygons per call beyond int32
 * indexing: E < 2^31, jobs < 2^31, H*W < 2^31.  SC_ERR_ARG, before any launch, for bad dims, a null pointer, an edge range outside
 * [0, E], a box that leaves the raster or a job0 that is not that running sum.  P = 0 or no job: out is cleared, nothing is
 * launched.  Work: sum over polygons of box rows x (edges + box columns / 64) -- meant for plumes (hundreds of polygons, boxes of
 * tens to hundreds of pixels), tolerable for a scene footprint (1e4 edges x 1e4 rows).  Integer atomics only (LDS xor, global
 * max); no work-group waits on another.                                                                                      */
typedef struct sc_rast_poly {
  int32_t e0, e1;                                 /* its edges: [e0, e1) of the edge array                         */
  int32_t r0, r1, c0, c1;                         /* clipped box: rows [r0, r1), columns [c0, c1)                  */
  int32_t job0, reserved;
} sc_rast_poly;
typedef struct sc_rast_args {
  const double* edges;                            /* [E][4] device: x0, y0, x1, y1; 16-byte aligned                */
  const sc_rast_poly* polys;                      /* [P] device                                                    */
  const sc_rast_poly* polys_host;                 /* [P] host, the same table                                      */
  const int32_t* values;                          /* [P] device, or NULL for 1..P                                  */
  int32_t* out;                                   /* [H][W] device                                                 */
  int64_t E;
  int32_t P, H, W, reserved;
} sc_rast_args;
int sc_rasterize_polygons(const sc_rast_args* a, sc_stream stream);

/* Cloud-Optimized GeoTIFF products (starcop_amd/cog.py: write_cog; the reference's georeader.save_cog): overview pyramid, TIFF
 * tiles and the search for empty tiles on the device.  An image is (nb, h, w), uint8 (elem_bytes 1) or float32 (4), 1 <= nb <= 4,
 * read in place through non-negative element strides: an (h, w, nb) interleaved view has col_stride = nb.  Samples are compared
 * and moved as BIT PATTERNS: with has_nodata, a sample whose bits equal nodata_bits is nodata (-0.0 is not 0.0).
 *   sc_overview_reduce  halves the image `levels` (1..3) times in one launch: dst[k] is dense (nb, ceil(h / 2^(k+1)),
 *       ceil(w / 2^(k+1))).  Pixel (r, c) of a level is made from pixels (2r + i, 2c + j), i, j in {0, 1}, of the level before
 *       that lie inside it; every band on its own.  A sample is valid unless it is NaN (float32) or nodata.
 *         SC_COG_AVERAGE float32: (float)(S / count), S the float64 sum of the valid samples in the order (0,0), (0,1), (1,0),
 *                                 (1,1) (a single sample is its own sum), one rounding per operation; none valid: nodata, or
 *                                 the NaN 0x7FC00000 without one.
 *                        uint8:   (2 S + count) / (2 count) in integers; none valid: nodata.
 *         SC_COG_NEAREST          the bits of pixel (2r, 2c).
 *         SC_COG_MODE    uint8:   the most frequent valid value, the smallest of equally frequent ones; none valid: nodata.
 *       Level k + 1 is computed from the stored bits of level k: a launch of three levels equals three launches of one.  A
 *       work-group owns an aligned 64 x 64 source block and keeps the intermediate levels in LDS.  16-byte loads where
 *       col_stride = 1, the run lies inside the image and its address is 16-byte aligned; 16-byte stores where the level's width
 *       is a multiple of the vector and dst[k] is 16-byte aligned; element accesses otherwise.
 *   sc_tiff_tile_flags  flags[tile] = 1 where every in-image sample of every band of the bs x bs tile (row-major tile order) has
 *       the bits of the fill value -- nodata_bits with has_nodata, else 0 -- and 0 otherwise.  Padding does not count.
 *   sc_tiff_pack_tiles  tile t with slots[t] >= 0 is written to out + slots[t] * bs * bs * nb * elem_bytes as TIFF tile bytes:
 *       [bs][bs][nb] chunky little-endian samples, zero beyond the image edge, then the predictor per tile row: 1 none; 2 (uint8)
 *       byte k of a row minus byte k - nb, modulo 256; 3 (float32, TIFF Technical Note 3) the 4 * bs * nb bytes of a row ordered
 *       by significance, most significant byte of every sample first, then byte k minus byte k - nb over the whole row.  Tiles
 *       with slot -1 are not touched.  The slot table is given twice, on the device for the kernel and on the host for the
 *       checks made before the launch: every slot is -1 or inside [0, n_slots), no slot is given twice, out_bytes holds
 *       n_slots tiles, and the device table is read back and compared (one stream synchronisation).  n_slots = 0 launches nothing.
 * bs is a multiple of 16 with bs * nb * elem_bytes <= 32768; out is 16-byte aligned.  Addresses are 64-bit.  SC_ERR_ARG, before
 * any launch, for anything else.  No floating-point atomics: two calls give identical bytes.                                      */
#define SC_COG_MAX_BANDS 4
enum sc_cog_resampling { SC_COG_AVERAGE = 0, SC_COG_NEAREST = 1, SC_COG_MODE = 2 };
typedef struct sc_cog_image {
  const void* data;                               /* element [0][0][0], device                                     */
  int32_t elem_bytes;                             /* 1 = uint8, 4 = float32                                        */
  int32_t nb, h, w;
  int64_t band_stride, row_stride, col_stride;    /* elements                                                      */
  int32_t has_nodata;
  uint32_t nodata_bits;                           /* bit pattern of the nodata value (low elem_bytes bytes)        */
} sc_cog_image;
typedef struct sc_overview_args {
  sc_cog_image src;
  int32_t resampling;                             /* enum sc_cog_resampling                                        */
  int32_t levels;                                 /* 1..3                                                          */
  void* dst[3];                                   /* dense (nb, h_k, w_k) per level, device                        */
} sc_overview_args;
typedef struct sc_tiff_pack_args {
  sc_cog_image src;
  int32_t bs, predictor;
  int32_t n_slots, reserved;
  const int32_t* slots;                           /* [tiles] device: slot of each tile, -1 = do not write          */
  const int32_t* slots_host;                      /* the same on the host                                          */
  void* out;                                      /* [n_slots][bs][bs][nb] samples, device                         */
  size_t out_bytes;
} sc_tiff_pack_args;
int sc_overview_reduce(const sc_overview_args* a, sc_stream stream);
int sc_tiff_tile_flags(const sc_cog_image* src, int bs, uint8_t* flags /*[tiles] device*/, sc_stream stream);
int sc_tiff_pack_tiles(const sc_tiff_pack_args* a, sc_stream stream);

/* Exact Euclidean distance transform of binary images, and disc morphology as a threshold on it (starcop_amd/morphology.py).
 * For a batch (N, H, W) the TARGETS are the pixels with mask != 0 (invert = 0) or mask == 0 (invert = 1); for every pixel p
 *     d2(p) = min over the targets t of the same image of (row_p - row_t)^2 + (col_p - col_t)^2
 * an int32, exact, 0 on targets; SC_EDT_FAR everywhere in an image without a target.  Pixels outside the image do not exist.
 * The mask is uint8, read in place through non-negative element strides: one band of an (H, W, 4) interleaved image has
 * stride_w = 4.  H, W <= 32767 (H^2 + W^2 fits an int32), H*W < 2^31, N <= 65535.  Outputs, dense [N][H][W], any non-empty subset:
 *   dist2   int32; with max_dist2 > 0 every value above it is written as SC_EDT_FAR
 *   dist    float32 (float)(sqrt((double)d2) * pixel_size), one rounding of the fp64 product; +inf where dist2 is SC_EDT_FAR
 *   within  uint8 d2 <= thresh2: the dilation by the disc {dy^2 + dx^2 <= thresh2} when the targets are the set pixels, the
 *           complement of the erosion (outside counted as set) when they are the unset ones; with `negate` d2 > thresh2, that
 *           erosion itself
 * Two row passes behind the entry point, bit-equal wherever both apply; sc_edt_variant is the rule (a pure host function):
 *   SC_EDT_WINDOW    when a cap is known -- max_dist2 (the larger of it and thresh2 when `within` is asked for too), or thresh2
 *                    when `within` is the only output -- and R = floor(sqrt(cap)) <= SC_EDT_WINDOW_MAX_R: minimum over the
 *                    2 R + 1 columns around the pixel, staged in LDS
 *   SC_EDT_ENVELOPE  otherwise: the lower envelope of parabolas per row, work independent of the distances
 * `variant` / `forced`: 0 the rule, or one of the two; SC_ERR_ARG for the window beyond its limit or without a cap.
 * work: 16-byte aligned device memory of sc_edt_call_workspace_bytes(a) bytes, the size THAT call needs (0 where sc_edt would
 * refuse its arguments): about 2.3 bytes per pixel of the batch for the window pass, about 10.3 for the envelope.
 * sc_edt_workspace_bytes(N, H, W) (0 for bad dims) is the larger of the two and serves any call.  thresh2 < SC_EDT_FAR, so that
 * an image without a target is within nothing.  4 launches (window) or 5 (envelope).  SC_ERR_ARG, before any launch, for bad dims, a null mask, no output, negative strides or caps, a
 * pixel_size <= 0 with `dist`, or a workspace that is too small.  No atomics: two calls give identical bytes.
 * sc_label_keep: out[n][i] = keep[n][labels[n][i]] for label values in [0, M], 0 outside -- the sieve's gather; keep is a
 * device table [N][M + 1] (entry 0 the background).                                                                          */
#define SC_EDT_FAR 0x7FFFFFFF
#define SC_EDT_WINDOW_MAX_R 64
enum sc_edt_row_pass { SC_EDT_WINDOW = 1, SC_EDT_ENVELOPE = 2 };
typedef struct sc_edt_args {
  const uint8_t* mask;                            /* element (0, 0) of image 0, device                             */
  int64_t stride_n, stride_h, stride_w;           /* elements (bytes) between images, rows, columns                */
  int32_t N, H, W;
  int32_t invert;                                 /* 0: targets are mask != 0; 1: mask == 0                        */
  int32_t max_dist2;                              /* 0: no cap                                                     */
  int32_t thresh2;                                /* for `within`                                                  */
  int32_t variant;                                /* 0, SC_EDT_WINDOW or SC_EDT_ENVELOPE                           */
  int32_t negate;                                 /* 1: `within` receives d2 > thresh2 instead                     */
  double pixel_size;                              /* for `dist`                                                    */
  int32_t* dist2;                                 /* [N][H][W] device outputs, each may be NULL                    */
  float* dist;
  uint8_t* within;
} sc_edt_args;
size_t sc_edt_workspace_bytes(int N, int H, int W);
size_t sc_edt_call_workspace_bytes(const sc_edt_args* a);
int sc_edt(const sc_edt_args* a, void* work, size_t work_bytes, sc_stream stream);
int sc_edt_variant(int H, int W, int max_dist2, int forced);
int sc_label_keep(const int32_t* labels, const uint8_t* keep /*[N][M+1]*/, uint8_t* out, int N, int M, int H, int W,
                  sc_stream stream);

/* Exact feature transform: WHICH target is the nearest one (starcop_amd/morphology.py: nearest_index, expand_labels,
 * fill_nearest; starcop_amd/plumes.py: background_rings).  Targets, dims, strides and the two row passes are sc_edt's; for every
 * pixel p, nearest(p) is the target minimising (row_p - row_t)^2 + (col_p - col_t)^2, AMONG EQUALLY NEAR TARGETS THE ONE WITH THE
 * SMALLEST COLUMN, THEN THE ONE WITH THE SMALLEST ROW.  That is what the separable scheme gives when the column pass prefers the
 * target above on a tie, the window scans left to right replacing on < only, and the envelope keeps the earlier parabola on
 * equality.  Outputs, dense [N][H][W], any non-empty subset:
 *   index   int32 row_t * W + col_t; a target's own index is itself; -1 wherever dist2 is SC_EDT_FAR (an image without a
 *           target, or with max_dist2 > 0 every pixel with d2 > max_dist2)
 *   dist2   int32, bit-equal to what sc_edt writes for the same mask, invert, max_dist2 and variant
 *   dst[i]  for i < n_planes <= SC_EDT_NEAREST_MAX_PLANES: dst[i][n][p] = src[i][n][nearest(p)], and the pixel's own word
 *           src[i][n][p] where index is -1.  A plane is 4-byte words (int32 labels, float32 values: copied as bits), dense H x W
 *           per image, src_stride[i] >= 0 words between images; dst[i] dense and not overlapping any source.
 * The row pass is sc_edt_variant(H, W, max_dist2, variant): the window when 0 < floor(sqrt(max_dist2)) <= SC_EDT_WINDOW_MAX_R.
 * max_dist2 = 0 means no cap (a cap of 0 pixels is the caller's: the targets themselves).  work: 16-byte aligned device memory
 * of sc_edt_nearest_call_workspace_bytes(a) bytes (0 where the call would refuse): sc_edt's layout for that row pass, and for
 * the envelope 2 more bytes per padded pixel (the winning columns, uint16, transposed beside the distances);
 * sc_edt_nearest_workspace_bytes(N, H, W) (0 for bad dims) serves any call.  Launches as sc_edt: 4 (window) or 5 (envelope); the
 * gathers are scattered 4-byte loads.  SC_ERR_ARG, before any launch, for everything sc_edt refuses and for n_planes outside
 * 0..8, a null or aliased plane pointer, a negative source stride.  No atomics: two calls give identical bytes.              */
#define SC_EDT_NEAREST_MAX_PLANES 8
typedef struct sc_edt_nearest_args {
  const uint8_t* mask;                            /* element (0, 0) of image 0, device                             */
  int64_t stride_n, stride_h, stride_w;           /* elements (bytes) between images, rows, columns                */
  int32_t N, H, W;
  int32_t invert;                                 /* 0: targets are mask != 0; 1: mask == 0                        */
  int32_t max_dist2;                              /* 0: no cap                                                     */
  int32_t variant;                                /* 0, SC_EDT_WINDOW or SC_EDT_ENVELOPE                           */
  int32_t n_planes;                               /* gathered planes, 0..SC_EDT_NEAREST_MAX_PLANES                 */
  int32_t reserved;
  int32_t* index;                                 /* [N][H][W] device outputs, each may be NULL                    */
  int32_t* dist2;
  const void* src[SC_EDT_NEAREST_MAX_PLANES];     /* [H][W] words per image, device                                */
  int64_t src_stride[SC_EDT_NEAREST_MAX_PLANES];  /* words between images                                          */
  void* dst[SC_EDT_NEAREST_MAX_PLANES];           /* [N][H][W] words, device                                       */
} sc_edt_nearest_args;
size_t sc_edt_nearest_workspace_bytes(int N, int H, int W);
size_t sc_edt_nearest_call_workspace_bytes(const sc_edt_nearest_args* a);
int sc_edt_nearest(const sc_edt_nearest_args* a, void* work, size_t work_bytes, sc_stream stream);

/* ------------------------------------------------------------------------- */
/* HOST functions (no device involved): decoders of the on-disk sample format -- one tiled GeoTIFF per product per sample,
 * read by rasterio in the reference (starcop/data/dataset.py:66-76, written by save_cog at sampling_dataset.py:332-355).
 *   sc_tiff_lzw_decode : TIFF 6.0 LZW (GDAL's default COG compression); *written = bytes produced (<= n_out)
 *   sc_tiff_unpredict  : undo TIFF predictor 2 (integer samples) or 3 (floating point) of one decoded block of
 *                        rows x cols x spp samples of bps bytes; `out` receives little-endian samples               */
int sc_tiff_lzw_decode(const uint8_t* in_host, size_t n_in, uint8_t* out_host, size_t n_out, size_t* written_host);
int sc_tiff_unpredict(const uint8_t* in_host, int predictor, int rows, int cols, int spp, int bps, int big_endian,
                      uint8_t* out_host);

#ifdef __cplusplus
}
#endif
#endif /* STARCOP_HIP_H */
