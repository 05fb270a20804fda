/* usot_hip.h — C ABI of libusot_hip.so: hand-written gfx950 (MI355X) kernels for the
 * USOT Siamese-tracking forward pass.
 *
 * Conventions (mirroring the reference's only native ABI,
 * lib/models/prroi_pool/src/prroi_pooling_gpu_impl.cuh:20-28):
 *   - the caller owns every buffer; kernels borrow raw DEVICE pointers for the duration
 *     of the enqueue; nothing is allocated or retained by the library (plans excepted);
 *   - every call enqueues asynchronously on the given hipStream_t (passed as void*);
 *   - every entry point returns 0 on success or a negative USOT_E* code — never exit()
 *     (the reference's launcher calls exit(-1), prroi_pooling_gpu_impl.cu:20-27);
 *   - all tensors are float32 unless a name says otherwise; "NHWC" = channels innermost.
 *
 * Each entry point cites the reference code it replaces.
 */
#ifndef USOT_HIP_H
#define USOT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USOT_OK            0
#define USOT_EINVAL       -1   /* bad shape / unsupported geometry */
#define USOT_ELAUNCH      -2   /* hipGetLastError() after launch   */
#define USOT_ENOMEM       -3
#define USOT_ESTATE       -4   /* plan used in the wrong state     */
#define USOT_ENOTBUILT    -5   /* a conv tile id that exists only in the -DUSOT_EXPERIMENTS build (usot_conv_tile_built) */

/* activation codes of the conv epilogue */
#define USOT_ACT_NONE      0
#define USOT_ACT_RELU      1
#define USOT_ACT_EXP       2   /* exp(x)                  connect.py:236-237 (bbox head)      */
#define USOT_ACT_CONF      3   /* exp(min(max(x,0),4))    connect.py:128-131 (ReLU then clamp) */

int usot_abi_version(void);
/* Launchers cache per-DEVICE state (zero pages, LDS-limit raises, CU counts) in tables indexed by the current HIP device:
 * usot_device_slot() = that index (hipGetDevice; 0 .. 15) or -1; usot_device_guard() = USOT_OK when the current device has a slot,
 * USOT_ESTATE otherwise.  One process may drive one GPU (the benchmarked form: one rank per GPU) or several (set the device, use its
 * streams); until round 6 the library bound itself to the first device it saw. */
int usot_device_slot(void);
int usot_device_guard(void);
/* HBM ceiling probe of the box (csrc/bw_probe.hip): mode 0 read `bytes`, 1 copy `bytes`, 2 read `bytes` + write bytes / 4
 * (GroupDW's byte mix, one interleaved read stream, non-temporal stores), 3 GroupDW's TRAFFIC without its compute - an address-level
 * emulation of the batched launch for S = bytes / (3 * 841 * 1024) samples: (sample, 64-channel group) blocks reading 256-byte
 * granules of three maps in src (S * 3 * 841 KiB) and writing S * 625 KiB to dst.  bytes % 4096 == 0 (mode 3: % 1024). */
int usot_bw_probe(void *stream, const void *src, void *dst, int64_t bytes, int mode);
const char *usot_strerror(int code);

/* ---- convolution as implicit GEMM on fp32 MFMA (v_mfma_f32_16x16x4_f32) -------------
 * y = act(conv(x, w) + bias [+ res]).  BatchNorm is folded into w/bias by the host.
 * Replaces every nn.Conv2d + nn.BatchNorm2d (+ReLU, +residual add) launch of
 * lib/models/modules.py:37-56,138-146 and lib/models/connect.py:19-53,110-119,178-215.
 *   x    NHWC  [N][H][W][Cin], Cin % 32 == 0
 *   w    packed [Cout][KH*KW*Cin], k = (kh*KW + kw)*Cin + ci
 *   y    NHWC  [N][OH][OW] with pixel stride y_cstride and channel offset y_coff, or
 *        NCHW  [N][Cout][OH][OW] when y_nchw != 0
 *   res  optional, laid out like an NHWC y with (res_cstride, res_coff)
 *   groups > 1 runs `groups` independent problems of identical geometry in one launch
 *   (pointer strides *_gs in elements): the three head towers, connect.py:178-207.
 *   act applies to channels [0, act_split) and act2 to [act_split, Cout) (act_split >= Cout
 *   means act everywhere): lets conf_gen|value_gen run as one Cout=512 conv.  Any act_split is exact; one that is
 *   not a multiple of 4 (with act != act2) takes the per-channel scalar epilogue instead of the 16-byte one, as do
 *   y_cstride / y_coff / res_cstride / res_coff / y_gs / r_gs / b_gs that are not multiples of 4 and y_nchw.
 *   y_cstride / res_cstride 0 = Cout (dense).  A launch writes y[m][y_coff .. y_coff + Cout) of every pixel and
 *   nothing else: convolutions may fill channel slices of one map side by side.
 *   ksplit > 1 splits the K loop over `ksplit` workgroups; partials go to `ws` and the LAST slice of a
 *   tile to arrive sums them (in slice order) and applies the epilogue inside the same launch.  `ws` holds
 *   usot_conv_ws_floats(d) floats — the slabs [ksplit][groups][M][Cout] followed by one ticket word per tile —
 *   and must be ZERO before its first use (the kernel leaves the tickets zero again).
 *   tile: 0 = heuristic, else one of USOT_TILE_* ids (see usot_conv_tile_count).
 */
typedef struct usot_conv_desc {
    const float *x, *w, *bias, *res;
    float *y;
    float *ws;
    int32_t N, H, W, Cin, OH, OW, Cout;
    int32_t KH, KW, stride, pad_h, pad_w, dil_h, dil_w;
    int32_t y_cstride, y_coff, res_cstride, res_coff, y_nchw;
    int32_t act, act2, act_split;
    int32_t groups;
    int64_t x_gs, w_gs, b_gs, y_gs, r_gs;
    int32_t ksplit, tile;
    int32_t w_frag;   /* 1: `w` is in MFMA fragment order (usot_conv_pack_wfrag_f32) — required by, and only valid with, the
                       * weight-streaming tiles (usot_conv_tile_wfrag(tile) == 1); row offsets / group strides of the bank must
                       * be multiples of 16 rows */
    int32_t defer;    /* with ksplit > 1: 1 = DEFERRED reduction - the launch writes its ksplit partial tiles [ksplit][groups][M][Cout]
                       * to `ws` (plain stores, no tickets) and applies NEITHER bias NOR activation; `y` is not written.  The consumer
                       * sums the slabs, adds the bias and activates while it stages its input (usot_pw_pair_desc.t2_parts).  A kernel
                       * boundary is the synchronisation: no in-launch combine (4-6 us on the tail of a 20 us launch), no second launch */
    const float *w_scale;   /* w_frag == 2 (the split-fp16 tiles, usot_conv_tile_wfrag(tile) == 2): `w` holds every filter row as hi + lo
                       * fp16 of (row x a power of two) - per k-tile of 64: 64 hi halves then 64 lo halves, the 256 bytes of the fp32 row
                       * segment - and w_scale[g * b_gs + co] = 1 / (that power of two x 8) multiplies the finished sums (8 = the
                       * activation scale the kernel applies before it splits them).  NULL otherwise. */
    int32_t x_split;  /* 1: `x` is a SPLIT map - per pixel and 64-channel block the 64 hi halves then the 64 lo halves (fp16) of 8 x value,
                       * the 256 bytes of the fp32 block - as written by a launch with y_split = 1.  Required by, and only valid with, the
                       * all-DMA split-fp16 tiles (usot_conv_tile_xsplit(tile) == 1): both operands then reach LDS by LDS-DMA */
    int32_t y_split;  /* 1: the result is written as a split map (split-fp16 tiles only; dense NHWC, Cout % 64 == 0, no residual, no
                       * split-K).  Its only readers are launches with x_split = 1 */
    int32_t *ovf;     /* split-fp16 tiles: NULL, or a device word the launch sets to 1 (sticky: it never clears it) when one of its finished
                       * sums is not finite - what an activation beyond the fp16 window (|x| >= 8 188: hi = inf, lo = -inf) or a non-finite
                       * input turns every sum it enters into - BEFORE bias / activation / split-K slabs see the sum (a ReLU would turn the
                       * NaN into a finite 0).  The caller re-runs the work on the exact-fp32 tiles (usot_amd/engine.py: Session, Engine.track) */
    const int32_t *n_dyn;   /* NULL (off), or a DEVICE word read by the launch: a run-time image count.  Images
                       * [0, clamp(*n_dyn - n_first, 0, N)) of this problem are computed; the rows of the others are neither read nor
                       * written (a tile that straddles the limit treats them as it treats rows past N * OH * OW; they never reach `ovf`),
                       * and a workgroup whose tile lies wholly past the limit leaves before it touches LDS, `ws` or a ticket.  `ws`, its
                       * slab strides and the ticket indices are those of the static N: every k-slice of a tile takes the same decision and
                       * the tickets stay zero.  Lets ONE captured launch serve a number of images decided on the device (the session's
                       * distinct memory rows, usot_rows_append_gather_dedupe_f32).  Producer / consumer tiles only (conv_igemm_f32_v3,
                       * exact-fp32 and split-fp16 - the ids with usot_conv_tile_dyn(tile) == 1), not with `defer`: USOT_EINVAL otherwise.
                       * In a batched launch the problems with the higher n_first should come last: their workgroups then own the
                       * highest block ids and the empty ones drain behind the working ones */
    int32_t n_first;  /* with n_dyn: the index, in the caller's image numbering, of this problem's first image (>= 0) */
} usot_conv_desc;

int usot_conv2d_f32(void *stream, const usot_conv_desc *d);
/* up to 4 convolutions of different geometry side by side in ONE launch (same tile shape =
 * d[0].tile, own ksplit each): shortcut conv + conv1 of a bottleneck, the three dilated
 * encoders of one input, the prediction heads. */
int usot_conv2d_batch_f32(void *stream, const usot_conv_desc *d, int n);
/* thin 3x3 / stride 1 / pad 1 convolutions with 1-4 output channels and NCHW output (the prediction
 * heads, connect.py:236-241,275): up to four descriptors of the same input geometry per launch, one
 * wavefront per output pixel; honours x, w, bias, y, N, H, W, Cin, Cout, act, groups and the group
 * strides of the descriptor.  From 1024 output rows (Cin = 256: batches of >= 14 streams) the launcher
 * switches to one wavefront per output ROW with the filters in registers and a sliding 3x3 window —
 * bit-identical results; d[0].tile = 70 forces the per-pixel form (tests). */
int usot_thin_conv3x3_f32(void *stream, const usot_conv_desc *d, int n);
int usot_plan_add_thin_conv(void *plan, const usot_conv_desc *d, int n);
int usot_conv_tile_count(void);
int usot_conv_tile_info(int tile, int *bm, int *bn);           /* tile ids are 1..count */
int usot_conv_tile_built(int tile);                            /* 1: compiled into this library (the routed tiles; every id with -DUSOT_EXPERIMENTS) */
int usot_experiments_built(void);                              /* 1: the library was built with -DUSOT_EXPERIMENTS */
int usot_conv_tile_name(int tile, char *buf, int len);         /* kernel symbol of the tile */
int usot_conv_tile_launch(int tile, int *threads, int *lds_bytes);   /* workgroup size and dynamic LDS of the tile; zeros: not built */
int usot_conv_tile_dyn(int tile);                              /* 1: the tile honours usot_conv_desc.n_dyn (run-time image count) */
int usot_conv_tile_xsplit(int tile);                           /* 1: the tile reads a split input map (usot_conv_desc.x_split) */
int usot_conv_tile_wfrag(int tile);                            /* 1: the tile streams its filters in fragment order; 2: split-fp16 bank + w_scale */
/* weight-stationary tiles (filters held in registers, k split over the 8 waves of a workgroup) serve ONE K each: returns it
 * (0: the tile takes any K); *kpanel = the multiple Cin must have (128 / 256).  They also need Cout % 32 == 0, ksplit == 1. */
int usot_conv_tile_kreq(int tile, int *kpanel);
/* persistent stream-K tiles (conv_igemm_f32_v3p): the launch is ONE resident set of workgroups that share the (tile, k-tile)
 * units of all its problems evenly; shares that end inside a tile meet through write-through slabs and per-wave tickets in
 * d[0].ws (usot_conv_streamk_ws_floats floats, zero before first use).  ksplit must be 1. */
int usot_conv_tile_streamk(int tile);
int64_t usot_conv_streamk_ws_floats(const usot_conv_desc *d, int n, int tile);
/* filter bank [Cout][K] (K % 64 == 0) -> ceil(Cout/16)*16*K floats in fragment order
 * [16-row block][k-tile of 64][round of 16 k][lane][4 k]; rows past Cout zero.  One launch, any stream. */
int usot_conv_pack_wfrag_f32(void *stream, const float *w, float *wf, int Cout, int K);
int64_t usot_conv_ws_floats(const usot_conv_desc *d);          /* workspace need for ksplit */

/* ---- bf16 variant for the batched backbone (BASELINE config 3): x / w / res / y are bf16
 * NHWC (uint16 storage), bias fp32, accumulate fp32 on v_mfma_f32_16x16x32_bf16.  Uses
 * N..dil_w, act (NONE | RELU), res, tile of the descriptor; dense output; Cin % 64 == 0,
 * Cout % 4 == 0.                                                                         */
int usot_conv2d_bf16(void *stream, const usot_conv_desc *d);
/* general low-precision form: dtype 0 = bf16, 1 = fp16 (v_mfma_f32_16x16x32_f16); out_f32 != 0
 * stores the result as fp32 (outputs feeding the fp32 xcorr / reduce / prediction convs, BASELINE
 * config 5).  Also honoured: act / act2 / act_split (NONE, RELU, EXP, CONF) and groups with x_gs,
 * w_gs, b_gs, y_gs (y_gs in OUTPUT elements; no residual with groups).  Not supported: ksplit,
 * y_nchw, channel-offset outputs.  tile: 0 = heuristic, 1..usot_conv_bf16_tile_count().
 * Unsupported fields are REJECTED, not ignored - USOT_EINVAL for y_coff != 0, res_coff != 0, y_cstride or res_cstride other
 * than 0 or Cout (y and res are dense [M][Cout]), and for 0 < act_split < Cout with act != act2 unless act_split % 8 == 0
 * (the epilogues choose the activation per 8 channels).  r_gs is not read (no residual with groups).                  */
int usot_conv2d_lp(void *stream, const usot_conv_desc *d, int dtype, int out_f32);
int usot_conv_bf16_tile_built(int tile);                       /* 1: the low-precision tile id is compiled into this library (cf. usot_conv_tile_built) */
int usot_conv_bf16_tile_info(int tile, int *bm, int *bn);      /* pixels x channels of a low-precision tile, ids 1..count (cf. usot_conv_tile_info; 0 x 0: not built) */
int usot_cvt_f32_to_lp(void *stream, const float *src, void *dst, int64_t n, int dtype);
int usot_maxpool3x3s2_lp(void *stream, const void *x, void *y, int N, int H, int W, int C, int OH, int OW, int dtype);
int usot_conv_bf16_tile_count(void);
/* fused low-precision stem (7x7/s2 conv + BN + ReLU) + 3x3/s2/p1 max-pool on the bf16|fp16 MFMA:
 * modules.py:70-74,138-141 in one launch.  wfrag: filter bank as MFMA A fragments [4][6][64][8].
 * The kernel convolves x - mu[ci]; bias must already contain sum_k w[co][k] * mu[ci(k)].
 * dtype 0: bf16 fragments, crop as hi + lo bf16 (two MFMAs per fragment), bf16 output; 1: fp16 throughout; 2: fp16
 * fragments and crop (11 significant bits on both operands, one MFMA per fragment), bf16 OUTPUT — the stem of the bf16
 * backbone (|x - mu| < 152 and BN-folded stem filters are far inside the fp16 range). */
int usot_stem_pool_lp(void *stream, const float *x, const void *wfrag, const float *bias, void *y,
                      int N, int H, int W, int OH, int OW, int PH, int PW, int dtype,
                      float mu0, float mu1, float mu2);
/* host only: the number of 4x8 pooled tiles a workgroup of usot_stem_pool_lp walks along x for a launch of this size
 * (4, 2 or 1: the longest strip that still leaves six workgroups per compute unit of a 256-CU device); 0 for N, PH or
 * PW < 1.  The launcher takes its strip from this function. */
int usot_stem_pool_lp_strip(int N, int PH, int PW);
int usot_cvt_f32_to_bf16(void *stream, const float *src, void *dst, int64_t n);
int usot_maxpool3x3s2_bf16(void *stream, const void *x, void *y, int N, int H, int W, int C, int OH, int OW);

/* ---- fused pair of pointwise convolutions of the low-precision backbone: a bottleneck's conv3 + BN + residual +
 * ReLU (modules.py:48-56) and the NEXT block's conv1 + BN + ReLU (modules.py:40-42; or the neck's 1x1, connect.py:
 * 294-300) in one persistent launch — the 4x-wide map Y is written once and never read back, the next tile's reads fly
 * under the second GEMM (csrc/pw_pair.hip).  All activations bf16|fp16 NHWC dense, fp32 accumulate, biases fp32:
 *   Y[M][CO] = relu(t2[M][CM] . w3^T + b3 + res[M][CO]);   T[M][CN] = act2(Y . w1^T + b1)
 * w3p and w1 are in the kernel's FRAGMENT order (every MFMA fragment load = one contiguous KiB): build them with
 * usot_pw_pair_layout, which lists for each packed 16-byte chunk the source (row, first k); b3 and b1 natural order.
 * Shapes: usot_pw_pair_supported(CM, CO, CN).  act2: USOT_ACT_NONE | USOT_ACT_RELU.  dtype 0 = bf16, 1 = fp16.     */
typedef struct usot_pw_pair_desc {
    const void *t2, *w3p, *res, *w1;
    const float *b3, *b1;
    void *y, *t;
    int32_t M, CM, CO, CN, act2;
    void *ws;             /* fp32 form only: usot_pw_pair_f32_ws_floats() zero-initialised floats, or NULL */
    /* fp32 form only: t2 given as t2_parts > 1 partial sums [t2_parts][M][CM] of the producing convolution (usot_conv_desc.defer);
     * the kernel stages relu(sum of the parts in order + t2_bias) as its pixel tile.  0 / 1: t2 is the finished map. */
    int32_t t2_parts, res_parts;
    const float *t2_bias;
    /* fp32 form only: res given as res_parts > 1 partial sums [res_parts][M][CO] of the shortcut convolution (defer); the kernel
     * adds (sum of the parts in order + res_bias) as the residual - no activation: the downsample branch has none */
    const float *res_bias;
    int32_t *ovf;         /* usot_pw_pair_f32s only: NULL or the sticky not-finite word of usot_conv_desc.ovf (checked on both GEMMs' sums) */
} usot_pw_pair_desc;
int usot_pw_pair_lp(void *stream, const usot_pw_pair_desc *d, int dtype);
int usot_pw_pair_layout(int CM, int CO, int CN, int which, int32_t *row, int32_t *k0);   /* which: 0 = w3, 1 = w1 */
int usot_pw_pair_supported(int CM, int CO, int CN);
int usot_plan_add_pw_pair(void *plan, const usot_pw_pair_desc *d, int dtype);   /* dtype 2: the fp32 form below */

/* one pointwise EXPANSION convolution of the batched low-precision backbone, pixel-stationary (csrc/pw_panel.hip: the
 * panel's X fragments in registers, W streamed through LDS once per 256 pixels, register epilogue in 32-byte pieces):
 * y[M][N] = act(x[M][K] . w^T + bias (+ res)); x, w ([N][K], the conv kernels' layout), res, y in the storage type
 * (dtype 0 = bf16, 1 = fp16), bias fp32 or NULL, res NULL or [M][N], act USOT_ACT_NONE | USOT_ACT_RELU.
 * Replaces the 1x1 convs of modules.py:48-56,108-113 at batch 64.  Shapes: usot_pw_panel_supported(K, N). */
int usot_pw_panel_lp(void *stream, const void *x, const void *w, const float *bias, const void *res, void *y,
                     int M, int K, int N, int act, int dtype);
int usot_pw_panel_supported(int K, int N);
int usot_pw_panel_pixels(int CM, int CO, int CN);      /* pixels per panel = per workgroup (CN = 0: single conv); 0 = unsupported */
int usot_pw_panel_min_pixels(int K, int N);           /* the smallest panel of the single convolution (used below 192 default panels) */
int usot_plan_add_pw_panel(void *plan, const void *x, const void *w, const float *bias, const void *res, void *y,
                           int M, int K, int N, int act, int dtype);
/* ... and the fused pair of usot_pw_pair_lp in that form: Y's sixteen channels per lane, rounded, are the B fragments of
 * the second GEMM (no LDS image of Y, no re-read from HBM).  Descriptor as for usot_pw_pair_lp EXCEPT that both banks
 * are in the conv kernels' natural layout: d->w3p = w3 [CO][CM], d->w1 = w1 [CN][CO]. */
int usot_pw_panel_pair_lp(void *stream, const usot_pw_pair_desc *d, int dtype);
int usot_pw_panel_pair_supported(int CM, int CO, int CN);
int usot_plan_add_pw_panel_pair(void *plan, const usot_pw_pair_desc *d, int dtype);

/* A bottleneck's conv2 -> conv3 of the batched low-precision backbone in ONE launch (csrc/conv_pw_lp.hip; modules.py:43-56):
 * y[M][4 CM] = relu(relu(conv(x; c2->w) + c2->bias) . w3^T + b3 + res[M][4 CM]).  c2 describes conv2 (x, w [CM][KH*KW*CM] in the
 * conv kernels' layout, bias, N, H, W, OH, OW, KH, KW, stride, pad, dil; Cin = Cout = CM, act = USOT_ACT_RELU; its y is IGNORED:
 * a panel of conv2's output stays in LDS and is consumed there), w3 [4 CM][CM], b3 fp32, res / y dense; storage type dtype 0 =
 * bf16, 1 = fp16.  Bit-identical to usot_conv2d_lp followed by usot_pw_panel_lp.  Shapes: usot_conv_pw_supported(Cin, CM, CO):
 * (256, 256, 1024) layer3, (128, 128, 512) layer2.  A workgroup owns a panel of usot_conv_pw_pixels(M) pixels: 256 (16
 * wavefronts), or 128 (8 wavefronts) when M gives fewer than 192 panels of 256 or a mostly empty second round of them (CUs < panels
 * < 1.5 CUs); c2->tile & 3 = 1 / 2 forces the 256 / 128 form.
 * 3 x 3 / stride 1 / pad = dil <= 4 convolutions run their k-loop ROW-SHARED (one staged activation tile per (kh, channel chunk)
 * serves the three kw taps; k order (kh, chunk, kw): same products, another fp32 summation order); c2->tile & 4 keeps the per-tap
 * loop, whose result is bit-identical to the unfused launches. */
int usot_conv_pw_lp(void *stream, const usot_conv_desc *c2, const void *w3, const float *b3, const void *res, void *y, int dtype);
int usot_conv_pw_supported(int Cin, int CM, int CO);
int usot_conv_pw_pixels(int64_t M);
/* ... and the pair form: the NEXT block's conv1 rides along as in usot_pw_panel_pair_lp, T[M][CN] = act2(Y . w1^T + b1) - a whole
 * bottleneck tail (conv2 -> conv3 + residual + ReLU -> next conv1) per launch.  d as for usot_pw_panel_pair_lp (w3p = w3 [CO][CM],
 * w1 [CN][CO], natural layouts; M = conv2's output pixels) except that d->t2 is ignored.  Bit-identical to usot_conv2d_lp followed
 * by usot_pw_panel_pair_lp.  Shapes: usot_conv_pw_pair_supported(CM, CO, CN): (128, 512, 128), layer2 - and (256, 1024, 256), layer3,
 * where the second convolution runs as a FIFTH phase instead (no registers for the pair form): the workgroup reads its own Y panel
 * back (L2 / Infinity Cache) and computes T as a 16-k-tile implicit GEMM on the freed LDS - T bit-identical to usot_conv2d_lp on Y. */
int usot_conv_pw_pair_lp(void *stream, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype);
int usot_conv_pw_pair_supported(int CM, int CO, int CN);
int usot_plan_add_conv_pw_pair(void *plan, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype);
int usot_plan_add_conv_pw(void *plan, const usot_conv_desc *c2, const void *w3, const float *b3, const void *res, void *y, int dtype);
/* usot_conv_pw_pair_lp for layer3's blocks (CM = 256, CO = 1024, CN = 256; conv2 3 x 3 / stride 1 / pad = dil in 1..4) with the matrix-pipe
 * work and the HBM work OVERLAPPED on every CU (csrc/conv_pw_ov.hip; modules.py:43-56,40-42): two kinds of 8-wave workgroup share a CU -
 * one runs conv2 on 128-pixel panels and, later, the next conv1 on the panel's Y rows; the other takes the conv2 panels (through L2), runs
 * conv3 + residual + ReLU and streams Y out - paired through write-through stores and flags in `ws`.  Same arithmetic as the pair form with
 * the row-shared k-loop (k order (kh, 32-channel chunk, kw)); T bit-identical to usot_conv2d_lp on this launch's Y.
 * ws: usot_conv_pw_ov_ws_bytes(M) bytes (M = conv2's output pixels), 16-byte aligned, ZERO before the first launch; every launch leaves the
 * hand-off flags zero again (graph-replay safe).  The word after the 2 ceil(M / 128) flags is a sticky error flag: non-zero = a bounded
 * hand-off wait ran out (the launch finished on garbage instead of hanging). */
int usot_conv_pw_ov_lp(void *stream, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype, void *ws);
int usot_conv_pw_ov_supported(int CM, int CO, int CN);
int64_t usot_conv_pw_ov_ws_bytes(int64_t M);
int usot_plan_add_conv_pw_ov(void *plan, const usot_conv_desc *c2, const usot_pw_pair_desc *d, int dtype, void *ws);
int usot_conv_pw_ov_trace(void *buf);      /* measurement: placement + phase time stamps of later launches into buf (32 int64 per workgroup); NULL = off */

/* 3x3 / stride 1 / pad 1 convolution of the batched low-precision backbone as a direct convolution from an LDS halo tile
 * (csrc/conv3x3_halo.hip; layer1's conv2 + BN + ReLU, modules.py:43-46): x, y NHWC dense [N][H][W][C] and w [Cout][9 Cin]
 * (k = (kh*3 + kw)*Cin + ci, the conv kernels' layout) in the storage type (dtype 0 = bf16, 1 = fp16), bias fp32 or NULL,
 * act USOT_ACT_NONE | USOT_ACT_RELU.  Shapes: usot_conv3x3_halo_supported(Cin, Cout) (64 -> 64). */
int usot_conv3x3_halo_lp(void *stream, const void *x, const void *w, const float *bias, void *y,
                         int N, int H, int W, int Cin, int Cout, int act, int dtype);
int usot_conv3x3_halo_supported(int Cin, int Cout);
int usot_plan_add_conv3x3_halo(void *plan, const void *x, const void *w, const float *bias, void *y,
                               int N, int H, int W, int Cin, int Cout, int act, int dtype);

/* Layer1's FIRST bottleneck of the batched low-precision backbone plus the next block's conv1 in ONE launch
 * (csrc/bneck_lp.hip; modules.py:37-58 with the 1x1 downsample of modules.py:108-113): the 64-channel intermediates stay in
 * LDS, the shortcut conv is the second half of conv3's k axis.  NHWC dense, storage type dtype 0 = bf16 | 1 = fp16:
 * x [N][H][W][64]; w1 [64][64]; w2 [64][576] (k = (kh*3 + kw)*64 + ci); w3c [256][128] = [conv3 | downsample] along k;
 * wn [64][256] (the next block's conv1); biases fp32 (BN folded; b3c = conv3's + the downsample's);
 * y [N][H][W][256] = relu(conv3(relu(conv2(relu(conv1 x)))) + downsample(x)), t [N][H][W][64] = relu(conv1'(y)).
 * At least eight 8 x 16 tiles (N * ceil(H/8) * ceil(W/16)).  Shapes: usot_bneck_first_supported(Cin, Cmid, Cout, Cnext). */
typedef struct usot_bneck_desc {
    const void *x, *w1, *w2, *w3c, *wn;
    const float *b1, *b2, *b3c, *bn;
    void *y, *t;
    int32_t N, H, W;
} usot_bneck_desc;
int usot_bneck_first_lp(void *stream, const usot_bneck_desc *d, int dtype);
int usot_bneck_first_supported(int Cin, int Cmid, int Cout, int Cnext);
int usot_plan_add_bneck_first(void *plan, const usot_bneck_desc *d, int dtype);
/* The REST of a layer1 bottleneck whose conv1 output already exists (the launch above, or this one, made it) + the next block's
 * conv1, one launch: conv2 3x3 + BN + ReLU, conv3 1x1 + BN + identity residual + ReLU (modules.py:43-58), then conv1' + BN + ReLU
 * of the following block (modules.py:40-42).  The descriptor's fields are read as: x = t1 [N][H][W][64] (this block's conv1
 * output), w1 = the RESIDUAL map [N][H][W][256] (the block's input), w2 [64][576], w3c = w3 [256][64], wn [Cnext][256],
 * b2, b3c (= conv3's bias), bn; b1 unused; y [N][H][W][256], t [N][H][W][Cnext].  Cnext 64 | 128. */
int usot_bneck_tail_lp(void *stream, const usot_bneck_desc *d, int Cnext, int dtype);
int usot_bneck_tail_supported(int Cmid, int Cout, int Cnext);
int usot_plan_add_bneck_tail(void *plan, const usot_bneck_desc *d, int Cnext, int dtype);

/* Channel-reducing 1x1 convolution of the batched low-precision backbone with the accumulators stationary and K streaming
 * (csrc/pw_kstream.hip; layer3's conv1 + BN + ReLU 1024 -> 256, modules.py:40-42, and the neck's 1x1 + BN, connect.py:294-300):
 * y[M][N] = act(x[M][K] . w^T + bias), x / w ([N][K]) / y in the storage type (dtype 0 = bf16, 1 = fp16), bias fp32 or NULL,
 * act USOT_ACT_NONE | USOT_ACT_RELU.  Shapes: usot_pw_kstream_supported(K, N) ((1024, 256)). */
int usot_pw_kstream_lp(void *stream, const void *x, const void *w, const float *bias, void *y, long M, int K, int N, int act, int dtype);
int usot_pw_kstream_supported(int K, int N);
int usot_plan_add_pw_kstream(void *plan, const void *x, const void *w, const float *bias, void *y, long M, int K, int N, int act, int dtype);

/* 3x3 convolutions with K = 9 Cin >= 2304 of the batched low-precision backbone in the same accumulator-stationary form
 * (csrc/conv_kstream.hip; layer3's shortcut conv and conv2, layer2's shortcut conv, modules.py:43-46,115-126): a lane is an
 * output pixel and fetches its MFMA B fragments straight from global memory three k-chunks ahead, W streams through LDS.
 * x, y NHWC dense, w [Cout][9 Cin] (k = (kh*3 + kw)*Cin + ci) in the storage type (dtype 0 = bf16, 1 = fp16), bias fp32 or
 * NULL, stride 1 | 2, pad <= dil, act USOT_ACT_NONE | USOT_ACT_RELU.  Shapes: usot_conv_kstream_supported (Cin 256 | 512,
 * Cout a multiple of 256, 3 x 3).  The batch must hold MORE than dil * (W + 1) pixels (N * H * W; USOT_EINVAL otherwise, for
 * a plan when the op runs): a lane parks a tap outside the image at most that far from the start of x. */
int usot_conv_kstream_lp(void *stream, const void *x, const void *w, const float *bias, void *y,
                         int N, int H, int W, int Cin, int Cout, int stride, int pad, int dil, int act, int dtype);
int usot_conv_kstream_supported(int Cin, int Cout, int KH, int KW);
int usot_plan_add_conv_kstream(void *plan, const void *x, const void *w, const float *bias, void *y,
                               int N, int H, int W, int Cin, int Cout, int stride, int pad, int dil, int act, int dtype);

/* the same pair in fp32 for the batch-1 frame (csrc/smallm_f32.hip; v_mfma_f32_16x16x4_f32, 16 pixels per workgroup):
 * every pointer of the descriptor is float32.  w3p / w1 in fragment order: the float at
 * [((cb * (K / 16) + r) * 64 + lane) * 4 + c] is W[cb * 16 + (lane & 15)][16 * r + 4 * (lane >> 4) + c]
 * (W = the [rows][K] filter bank: K = CM for w3p, CO for w1).  Shapes: usot_pw_pair_f32_supported.
 * With few pixel tiles (layer2 at batch 1-2) S = 4 workgroups share a tile, each owning a quarter of CO, and meet in
 * d->ws (write-through slabs + a ticket per tile, as the in-launch split-K of the conv kernels): size from
 * usot_pw_pair_f32_ws_floats (0 = not needed), zero before the first launch, owned by the caller; NULL = unsliced. */
int usot_pw_pair_f32(void *stream, const usot_pw_pair_desc *d);
int usot_pw_pair_f32_supported(int CM, int CO, int CN);
/* The same pair on SPLIT-fp16 operands (csrc/smallm_f32.hip: GemmRing BLO > 0; the arithmetic of the split-fp16 conv tiles): d->w3p and
 * d->w1 are the banks pre-split by the host - per column block of 16 rows and 32-k step a hi fragment (lane (quad, row) = 8 halves of
 * row x 2^e, k = 32 step + 8 quad ..) then the lo fragment, followed by the bank's per-row factors 1 / (2^e x 8) as floats - and the
 * kernel splits the staged pixel tile and its Y tile itself (x 8).  dtype 3 of usot_plan_add_pw_pair.  Shape (256, 1024, 256), sliced. */
int usot_pw_pair_f32s(void *stream, const usot_pw_pair_desc *d);
int usot_pw_pair_f32s_supported(int CM, int CO, int CN);
int64_t usot_pw_pair_f32_ws_floats(int M, int CM, int CO, int CN);

/* one pointwise convolution of the fp32 frame in the same style (16 pixels per workgroup, the pixel tile in LDS, filters
 * streamed from L2 in the fragment order above; several workgroups per pixel tile, each owning output channels):
 * y[M][N] = act(x[M][K] . W^T + b (+ res)), all float32 dense, act USOT_ACT_NONE | USOT_ACT_RELU, res may be NULL.   */
int usot_pw_single_f32(void *stream, const float *x, const float *wp, const float *b, const float *res, float *y,
                       int M, int K, int N, int act);
int usot_pw_single_f32_supported(int K, int N);
/* a whole bottleneck tail in one launch (layer1 of the fp32 frame): conv2 (3x3 / stride 1) + BN + ReLU on the im2col pixel
 * tile, then the pair of usot_pw_pair_f32 on its output without leaving the CU.  x NHWC [Nb][H][W][Cin] (conv1's output);
 * w2p conv2's packed bank [CM][9 Cin] in fragment order; d as for usot_pw_pair_f32 (d->t2 and d->ws ignored,
 * d->M = Nb * OH * OW).                                                                                               */
int usot_pw_triple_f32(void *stream, const float *x, const float *w2p, const float *b2, const usot_pw_pair_desc *d,
                       int Nb, int H, int W, int Cin, int OH, int OW, int pad_h, int pad_w, int dil_h, int dil_w);
int usot_pw_triple_f32_supported(int Cin, int CM, int CO, int CN);
int usot_plan_add_pw_triple(void *plan, const float *x, const float *w2p, const float *b2, const usot_pw_pair_desc *d,
                            int Nb, int H, int W, int Cin, int OH, int OW, int pad_h, int pad_w, int dil_h, int dil_w);

/* 3x3 / stride-1 convolution in that form (the pixel tile is the 16 x 9 Cin im2col image, zeros for padding taps):
 * x NHWC [Nb][H][W][Cin] dense, wp the packed bank [N][9 Cin] in fragment order, y [Nb * OH * OW][N] (+ res of that shape). */
int usot_stream_conv3x3_f32(void *stream, const float *x, const float *wp, const float *b, const float *res, float *y,
                            int Nb, int H, int W, int Cin, int OH, int OW, int N, int pad_h, int pad_w, int dil_h, int dil_w,
                            int act);
int usot_stream_conv3x3_f32_supported(int Cin, int N);
int usot_plan_add_stream_conv3x3(void *plan, const float *x, const float *wp, const float *b, const float *res, float *y,
                                 int Nb, int H, int W, int Cin, int OH, int OW, int N, int pad_h, int pad_w, int dil_h, int dil_w,
                                 int act);
int usot_plan_add_pw_single(void *plan, const float *x, const float *wp, const float *b, const float *res, float *y,
                            int M, int K, int N, int act);

/* ---- stem: 7x7 / stride 2 / pad 0 conv, 3 -> 64 channels, + folded BN + ReLU ---------
 * modules.py:70-72,138-140.  x NCHW [N][3][H][W] (the API-edge crop, BGR 0..255),
 * w packed [147][64] with row = (ci*7 + kh)*7 + kw, y NHWC [N][OH][OW][64].            */
int usot_stem_conv_f32(void *stream, const float *x, const float *w, const float *bias,
                       float *y, int N, int H, int W, int OH, int OW);
/* the same on x - mu[ci] (exact for this pad-0 conv; `bias` must then carry + sum_k w[k][co] * mu[ci(k)], folded in
 * float64 by the caller): raw crops sit around ~100, and the 147-tap float32 chain of every output otherwise rides on
 * 100 * sum(w).  mu = 0 is usot_stem_conv_f32.  N <= 65535 (one grid plane per image), as in the fused forms. */
int usot_stem_conv_mu_f32(void *stream, const float *x, const float *w, const float *bias,
                          float *y, int N, int H, int W, int OH, int OW, float mu0, float mu1, float mu2);

/* ---- max-pool 3x3 / stride 2 / pad 1 on NHWC (modules.py:74,141) ------------------- */
int usot_maxpool3x3s2_f32(void *stream, const float *x, float *y,
                          int N, int H, int W, int C, int OH, int OW);

/* ---- depthwise cross-correlation, NCHW planes (drop-in for xcorr_depthwise,
 * lib/models/connect.py:147-157): out[p][i][j] = sum_uv x[p][i+u][j+v] * k[p][u][v]
 * for P = B*C planes; one wavefront per plane pair, template tile in LDS, window taps
 * exchanged between lanes with DPP/shuffles.  Wx <= 64.                                */
int usot_xcorr_depthwise_f32(void *stream, const float *x, const float *k, float *out,
                             int P, int Hx, int Wx, int Hk, int Wk);

/* ---- its two gradients (csrc/xcorr_grad.hip), dout [P][Hx-Hk+1][Wx-Wk+1]:
 *   dx[p][a][b] = scale * sum_uv dout[p][a-u][b-v] * k[p][u][v]      (terms outside dout are 0)
 *   dk[p][u][v] = scale * sum_ij dout[p][i][j]     * x[p][i+u][j+v]
 * Every element is written once with a plain store (no atomics, no memset, no workspace) and every sum has a
 * fixed order: equal inputs give equal bits.  5x5 / 3x5 / 5x3 templates with Wx <= 64 run one wavefront per
 * plane (two planes per wavefront when Wx <= 32); anything else takes a one-thread-per-element kernel.
 * Same argument checks as the forward; P == 0 is a no-op.                                              */
int usot_xcorr_depthwise_bwd_x_f32(void *stream, const float *dout, const float *k, float *dx,
                                   int P, int Hx, int Wx, int Hk, int Wk, float scale);
int usot_xcorr_depthwise_bwd_k_f32(void *stream, const float *dout, const float *x, float *dk,
                                   int P, int Hx, int Wx, int Hk, int Wk, float scale);

/* ---- gradients of the fp32 convolution (csrc/conv_grad.hip).  The convolution is the one usot_conv_desc describes, groups = 1,
 * no residual, no activation, with the forward's layouts:
 *   x    NHWC  [N][H][W][Cin], Cin % 32 == 0
 *   w    packed [Cout][K], K = KH*KW*Cin, k = (kh*KW + kw)*Cin + ci
 *   dy   dense NHWC [N][OH][OW][Cout], the gradient of the convolution's output; m = (n*OH + oh)*OW + ow, M = N*OH*OW
 *   dw[co][k]       = sum_m dy[m][co] * x[n][oh*stride - pad_h + kh*dil_h][ow*stride - pad_w + kw*dil_w][ci]   (taps outside x are 0)
 *   db[co]          = sum_m dy[m][co]
 *   dx[n][h][w][ci] = sum over (co, kh, kw) and the output pixels whose tap (kh, kw) is x[n][h][w] of dy[m][co] * w[co][k]
 * Every pointer a launch uses must be 16-byte aligned.  Outputs are written once per element with plain stores: no atomics,
 * nothing has to be cleared, and every sum has an order fixed by the code, so equal inputs (and an equal psplit) give equal bits.
 *
 * usot_conv2d_wgrad_f32 (needs x, dy, dw; db NULL = not computed) runs on v_mfma_f32_16x16x4_f32 with the pixel index as the
 *   reduction axis.  A workgroup owns a tile of dw - *bco channels x *bk filter elements (usot_conv2d_wgrad_geometry) - and one of
 *   `psplit` slices of the pixels, slice s = [M*s/psplit, M*(s+1)/psplit), which it walks in steps of *chunk pixels.
 *   Summation order of one element: the pixels of a step ascending in one fmaf chain that starts at 0; steps ascending, each
 *   added to the slice's running total; then, with psplit > 1, the slices ascending (a second launch that reads the workspace).
 *   db: pixels of a step ascending, steps ascending, slices ascending.
 *   psplit 0 = the launcher's choice, usot_conv2d_wgrad_psplit(d): about four workgroups per compute unit of the current device,
 *   no slice shorter than two steps, at most 32.  psplit > M is an error.
 *   ws: usot_conv2d_wgrad_ws_floats(d) floats = psplit*Cout*(K + 1) - the slabs [psplit][Cout][K], then [psplit][Cout] partial
 *   sums of db - or 0 (ws may be NULL) when the split is 1.  Its contents before the launch do not matter.
 * usot_conv2d_dgrad_f32 (needs dy, w, dx) has two routes; usot_conv2d_dgrad_route(d) names the one a launch of d takes.
 *   Route A (1): stride 1, Cout % 32 == 0, pad <= dil*(K-1) in both directions and wt != NULL.  dx is then the forward convolution
 *   of dy with the bank rotated by 180 degrees and transposed, wt[ci][(kh*KW + kw)*Cout + co] = w[co][((KH-1-kh)*KW + KW-1-kw)*Cin + ci]
 *   (usot_conv_pack_dgrad_f32 writes it), at padding dil*(K-1) - pad: the launch IS usot_conv2d_f32 on (dy, wt), heuristic tile,
 *   its summation order.  route = 0 takes route A when it is open, and route B when it is not or when usot_conv2d_f32 answers
 *   USOT_EINVAL for that descriptor; route = 1 insists (USOT_EINVAL when closed); route = 2 forces route B.
 *   Route B (2): any stride and Cout; one thread per four channels of a dx pixel; per tap and block of 64 output channels an fmaf
 *   chain over co ascending, the chains added in (kh, kw, block) order.
 * Both launchers answer USOT_EINVAL, before they touch the device, for: a NULL pointer they need, a negative N, any other size
 * (H, W, Cin, OH, OW, Cout, KH, KW, stride, dil) below 1, a negative pad, Cin % 32 != 0, OH / OW that are not the convolution's,
 * psplit < 0 or > M, ws == NULL with a split above 1, a misaligned pointer.  N == 0 is a no-op that returns 0.  The host-only
 * queries answer USOT_EINVAL for a descriptor whose geometry the launchers would reject. */
typedef struct usot_conv_grad_desc {
    const float *x, *w, *wt, *dy;   /* wt: rotated bank for route A, or NULL */
    float *dx, *dw, *db, *ws;       /* NULL output = not wanted */
    int32_t N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad_h, pad_w, dil_h, dil_w;
    int32_t psplit;                 /* 0 = launcher's choice */
    int32_t route;                  /* dgrad: 0 = auto, 1 = force route A (USOT_EINVAL if not eligible), 2 = force route B */
} usot_conv_grad_desc;
int     usot_conv2d_wgrad_f32(void *stream, const usot_conv_grad_desc *d);       /* dw, db */
int     usot_conv2d_dgrad_f32(void *stream, const usot_conv_grad_desc *d);       /* dx */
int64_t usot_conv2d_wgrad_ws_floats(const usot_conv_grad_desc *d);               /* host only; for psplit = 0 the launcher's own choice */
int     usot_conv2d_wgrad_psplit(const usot_conv_grad_desc *d);                  /* host only: the split a psplit = 0 launch takes */
int     usot_conv2d_wgrad_geometry(int *bco, int *bk, int *chunk);               /* host only: Cout block, k block, pixels staged per step */
int     usot_conv_pack_dgrad_f32(void *stream, const float *w, float *wt, int Cout, int Cin, int KH, int KW);
int     usot_conv2d_dgrad_route(const usot_conv_grad_desc *d);                   /* host only: 1 = route A, 2 = route B */

/* ---- BatchNorm2d on NHWC fp32 maps, forward and gradients (csrc/batchnorm.hip; every nn.BatchNorm2d of connect.py, with the
 * ReLU that follows most of them).  A map is [M][C], M = N*H*W rows of C channels, C % 4 == 0 (every access is 16 bytes).
 *   training: mean[c] = sum_m x[m][c] / M,  var[c] = sum_m (x[m][c] - mean[c])^2 / M  (biased),  invstd = 1 / sqrt(var + eps)
 *   eval:     mean = running_mean,          invstd = 1 / sqrt(running_var + eps)
 *   xhat = (x - mean) * invstd,   pre = fma(xhat, gamma, beta),   y = act ? max(pre, 0) : pre
 *   dy' = act ? dy * (pre > 0) : dy;   dbeta[c] = sum_m dy'[m][c];   dgamma[c] = sum_m dy'[m][c] * xhat[m][c]
 *   dx = gamma * invstd * (dy' - dbeta / M - xhat * dgamma / M)  in training,   gamma * invstd * dy'  in eval
 * The backward pass recomputes `pre` from x with the forward's own instructions (it never reads y), so its mask is the sign of
 * the forward's output bit for bit; it therefore needs x, gamma, beta (with act) and the statistics the forward used.
 * Reductions run over `slices` ranges of row steps (a step is *rows rows, usot_batchnorm_geometry; slice s owns the steps
 * [steps*s/slices, steps*(s+1)/slices), steps = ceil(M / *rows), so a slice may own no row at all) times blocks of *chans
 * channels; each workgroup leaves its partial - (mean, M2) of its rows, or the two sums - in ws[slice][2][C] with plain stores,
 * and the second launch (normalise / dx) combines the slices of its channels in slice order (Chan's formula on (count, mean,
 * M2), counts from the geometry; slices without rows are never read).  No atomics; every sum has an order fixed by
 * (M, C, slices): equal inputs give equal bits.  Launches: forward training 2, forward eval 1, backward 2 - or 1 for an eval
 * call that wants dx only (no reduction), and the second is a single row of workgroups when dx is not wanted.
 * A launch writes its outputs and ws[0 .. usot_batchnorm_ws_floats) and nothing else; x, dy, gamma, beta are only read.
 * USOT_EINVAL, before the device is touched and with every output unwritten: d NULL, M < 1 (M < 2 in training: the unbiased
 * variance divides by M - 1), C < 4 or C % 4 != 0, training / act outside {0, 1}, slices < 0 or > M, eps negative or not
 * finite, a NULL pointer the call needs, a misaligned pointer (16 bytes). */
typedef struct usot_bn_desc {
    const float *x;                 /* [M][C] input map; both entry points */
    const float *gamma, *beta;      /* [C] affine; forward: both; backward: gamma, and beta when act = 1 (the mask) */
    float *running_mean;            /* [C]; training forward: updated in place when non-NULL, r = (1 - momentum) r + momentum mean; */
    float *running_var;             /*      the variance with the unbiased estimate var * M / (M - 1).  eval: read only, required */
    float *y;                       /* [M][C] forward output; the backward pass does not read it */
    float *save_mean, *save_invstd; /* [C]; training: written by the forward, read by the backward; unused in eval */
    const float *dy;                /* [M][C] gradient of y; backward only */
    float *dx;                      /* [M][C]; NULL = not wanted */
    float *dgamma, *dbeta;          /* [C]; NULL = not wanted */
    float *ws;                      /* usot_batchnorm_ws_floats(d) floats; contents before the call do not matter; may be NULL for the
                                     * launches without a reduction (eval forward, eval backward of dx alone) */
    int32_t M, C;                   /* rows (N*H*W) and channels */
    float eps, momentum;
    int32_t training;               /* 0 = running statistics, 1 = batch statistics */
    int32_t act;                    /* USOT_ACT_NONE | USOT_ACT_RELU */
    int32_t slices;                 /* row slices of the reductions; 0 = the launcher's choice (usot_batchnorm_slices) */
} usot_bn_desc;
int     usot_batchnorm_fwd_f32(void *stream, const usot_bn_desc *d);             /* y; training: save_*, running_* */
int     usot_batchnorm_bwd_f32(void *stream, const usot_bn_desc *d);             /* dx, dgamma, dbeta: the ones that are non-NULL */
int64_t usot_batchnorm_ws_floats(const usot_bn_desc *d);                         /* host only: 2 * slices * C (either entry point) */
int     usot_batchnorm_slices(const usot_bn_desc *d);                            /* host only: the split a slices = 0 launch takes */
int     usot_batchnorm_geometry(int *rows, int *chans);                          /* host only: rows per step, channels per workgroup */

/* ---- BatchNorm2d with a residual operand, forward and gradients (csrc/batchnorm.hip; the tail of a ResNet bottleneck,
 * out = relu(bn3(conv3(.)) + residual), modules.py:48-56).  Maps, statistics, slices and workspace are usot_bn_desc's; res and
 * dres are [M][C] like x.
 *   pre as in usot_bn_desc;   s = pre + res  (one float32 add, not contracted);   y = act ? max(s, 0) : s
 *   dy' = act ? dy * (s > 0) : dy;   dres = dy';   dgamma, dbeta and dx as in usot_bn_desc with this dy'
 * The statistics do not see the residual.  The backward pass recomputes s from x, res and the statistics the forward used, with
 * the forward's own instructions (it never reads y): its mask is the sign of the forward's output bit for bit.  res is read for
 * the mask only (act = 1), but is required in every call.
 * Workspace: usot_batchnorm_ws_floats(&d->bn).  Launches as for usot_bn_desc: forward training 2, eval 1; backward 2 - or 1 when
 * no reduction is needed: eval mode wanting only dx and / or dres, or any mode wanting only dres.
 * A launch writes its outputs and the workspace and nothing else.  No output may alias an input (y or dres on res, dx on x ...):
 * a workgroup reads rows that another may already have written.  Outputs may not alias each other either.
 * USOT_EINVAL, before the device is touched and with every output unwritten: every case of usot_bn_desc, res NULL, a misaligned
 * res or dres (16 bytes), a backward call that wants nothing (dx, dgamma, dbeta and dres all NULL). */
typedef struct usot_bn_add_desc {
    usot_bn_desc bn;                /* everything as documented for usot_bn_desc */
    const float *res;               /* [M][C] residual, required */
    float *dres;                    /* [M][C] gradient of res; NULL = not wanted */
} usot_bn_add_desc;
int     usot_batchnorm_add_fwd_f32(void *stream, const usot_bn_add_desc *d);     /* y; training: save_*, running_* */
int     usot_batchnorm_add_bwd_f32(void *stream, const usot_bn_add_desc *d);     /* dx, dgamma, dbeta, dres: the non-NULL ones */

/* ---- Conf_Fusion on separate confidence and value maps, forward and gradients (csrc/head_grad.hip; connect.py:123-144 behind
 * unfolded, training-mode BatchNorms - the inference engine's usot_conf_fusion_reduce_* work on the interleaved [conf | value]
 * layout of folded convs and have no gradient).  conf and value are NHWC maps [B*M][P][C] (P = H*W pixels, C % 4 == 0: every
 * access is 16 bytes), map b*M + m being memory slot m of batch element b; out and dout are [B][P][C].
 *   e_m = exp(min(max(conf_m, -6), 4)),   S = sum_m e_m  (m = 0 .. M-1, in that order),   w_m = e_m / S
 *   out = sum_m w_m * value_m             (in m order: the reference's association - normalise, then weight, then add)
 *   dvalue_m = w_m * dout,                dconf_m = [-6 <= conf_m <= 4] * w_m * (value_m - out) * dout
 * The clamp mask is inclusive (torch.clamp's gradient).  The backward pass recomputes e, S and out from conf and value: nothing
 * but the two inputs is saved.  e_m and S are the forward's, bit for bit; `out` is re-formed in float64 from the same e_m,
 * because value_m - out cancels when one weight dominates (M = 1: exactly 0).  One launch per call, one f32x4 lane per (b, p, c/4).
 * Algorithmic traffic: forward (2M + 1) * B*P*C*4 bytes, backward (4M + 1) * B*P*C*4 bytes (value is not read when dconf is not
 * wanted).  A launch writes its outputs and nothing else; conf, value and dout are only read.
 * USOT_EINVAL, before the device is touched and with every output unwritten: d NULL, B, M or P < 1, C < 4 or C % 4 != 0, a NULL
 * pointer the call needs (forward: conf, value, out; backward: conf, dout, and value with dconf), a misaligned pointer (16 bytes).
 * A backward call that wants neither gradient is USOT_OK without a launch. */
typedef struct usot_conf_fusion_desc {
    const float *conf, *value;      /* [B*M][P][C] inputs; both entry points */
    float *out;                     /* [B][P][C] forward output; the backward pass does not read it */
    const float *dout;              /* [B][P][C] gradient of out; backward only */
    float *dconf, *dvalue;          /* [B*M][P][C]; NULL = not wanted */
    int32_t B, M, P, C;             /* batch, memory slots per batch element, pixels per map, channels */
} usot_conf_fusion_desc;
int     usot_conf_fusion_fwd_f32(void *stream, const usot_conf_fusion_desc *d);  /* out */
int     usot_conf_fusion_bwd_f32(void *stream, const usot_conf_fusion_desc *d);  /* dconf, dvalue: the ones that are non-NULL */

/* ---- the box epilogue y = exp(adjust * p + bias[c]) with its gradients (csrc/head_grad.hip; connect.py:236-237 with `adjust`
 * and `bias` as learnable parameters - the inference engine fuses it into a folded conv as USOT_ACT_EXP).  p, y, dy and dp are
 * [R][4] (R = N*H*W rows of the bbox_pred conv's NHWC output); adjust (1 float) and bias (4 floats) are read from DEVICE memory.
 *   y[r][c] = exp(fma(adjust, p[r][c], bias[c]))
 *   g = dy * y  (y recomputed from p),   dp = adjust * g,   dbias[c] = sum_r g[r][c],   dadjust = sum_{r,c} g[r][c] * p[r][c]
 * Each workgroup of the backward launch sums its rows in a fixed tree and leaves five partials in ws[workgroup][5] with plain
 * stores; a second launch of one workgroup merges the partials in float64 in an order fixed by R.  No atomics: equal inputs give
 * equal bits.  Launches: forward 1; backward 2, or 1 when only dp is wanted (no reduction, ws may be NULL).
 * A launch writes its outputs and ws[0 .. usot_box_exp_ws_floats) and nothing else; p, dy, adjust and bias are only read.
 * USOT_EINVAL, before the device is touched and with every output unwritten: d NULL, R < 1, C != 4, a NULL pointer the call needs
 * (forward: p, adjust, bias, y; backward: p, adjust, bias, dy, and ws with dadjust or dbias), a misaligned pointer (16 bytes).  A
 * backward call that wants nothing is USOT_OK without a launch. */
typedef struct usot_box_exp_desc {
    const float *p;                 /* [R][4] input; both entry points */
    const float *adjust, *bias;     /* 1 and 4 floats in device memory; both entry points */
    float *y;                       /* [R][4] forward output; the backward pass does not read it */
    const float *dy;                /* [R][4] gradient of y; backward only */
    float *dp;                      /* [R][4]; NULL = not wanted */
    float *dadjust, *dbias;         /* 1 and 4 floats; NULL = not wanted */
    float *ws;                      /* usot_box_exp_ws_floats(d) floats; contents before the call do not matter */
    int32_t R, C;                   /* rows, and channels: 4 */
} usot_box_exp_desc;
int     usot_box_exp_fwd_f32(void *stream, const usot_box_exp_desc *d);          /* y */
int     usot_box_exp_bwd_f32(void *stream, const usot_box_exp_desc *d);          /* dp, dadjust, dbias: the ones that are non-NULL */
int64_t usot_box_exp_ws_floats(const usot_box_exp_desc *d);                      /* host only: 5 * ceil(R / 256) */

/* ---- fused SGD step over every tensor of an optimiser in ONE launch (csrc/sgd.hip; the reference's scripts/train_usot.py:
 * SGD with momentum 0.9 and weight decay 1e-4 over three parameter groups, behind `if is_valid_number(loss.item())`).
 * All values are fp32; per element of a tensor, with the tensor's own lr, weight_decay, momentum, grad_scale and flags:
 *   g'   = maximize ? -g : g
 *   d    = g' + weight_decay * p
 *   buf' = first ? d : momentum * buf + grad_scale * d      (momentum != 0; grad_scale = 1 - dampening)
 *   step = momentum == 0 ? d : nesterov ? d + momentum * buf' : buf'
 *   p'   = p - lr * step
 * The compiler may fuse multiply-adds.  The host forms 1 - dampening in double and rounds it to fp32 once.  With `first` set
 * buf is not read; with momentum == 0 buf is neither read nor written and may be NULL.  One pass: p, g and buf read, p and buf
 * written - 20 bytes per element (24 with zero_grads).
 *
 * The kernel reads a DEVICE-resident table: T records of usot_sgd_tensor followed by a chunk list of n_chunks entries
 * {int32 tensor, int32 chunk_in_tensor}; a chunk is usot_sgd_chunk_elems() consecutive elements of one tensor (a compile-time
 * multiple of 4 floats), the last chunk of a tensor is short, and a tensor with n == 0 has no chunk.  One workgroup handles one
 * chunk and strides over the chunk list by the grid, which is min(n_chunks, usot_sgd_grid_cap()) workgroups.  A tensor whose p, g
 * and buf (where it has one) are all 16-byte aligned is moved with 16-byte loads and stores and a scalar n % 4 tail; any other
 * tensor takes the scalar path as a whole.  The choice is per tensor, so it is uniform over a workgroup.
 *
 * usot_sgd_table_bytes and usot_sgd_table_fill are host functions and touch no device: the first sizes the table image for
 * the element counts n[0 .. T) and leaves the chunk count in *n_chunks (which may be NULL), the second validates the records
 * and writes the image into HOST memory - the caller uploads it.  usot_sgd_table_bytes answers USOT_EINVAL for a NULL n, T < 1,
 * a negative n[i] or more than 2^31 - 1 chunks.  usot_sgd_table_fill answers USOT_EINVAL, with the image untouched, for: t or
 * image NULL, T < 1; p or g NULL; buf NULL with momentum != 0; a pointer that is not 4-byte aligned; n < 0; a non-finite or
 * negative lr, weight_decay or momentum; a non-finite grad_scale; nesterov with momentum == 0 or grad_scale != 1; flag bits
 * other than the three below; `bytes` below usot_sgd_table_bytes.  `reserved` is written as 0 whatever it held: equal records
 * give equal images, byte for byte.
 *
 * usot_sgd_step_f32 launches once (not at all for n_chunks == 0, which is USOT_OK).  USOT_EINVAL before the device is touched:
 * d or table NULL, a table that is not 8-byte aligned, a guard or counters that is not 4-byte aligned, T < 1, n_chunks < 0 or
 * above 2^31 - 1.  T and n_chunks must be the ones
 * the uploaded image was made with.
 *   guard     NULL, or one float in device memory (the loss) that every workgroup reads.  When it is NaN, +-Inf or > 1e4 the
 *             launch writes no p and no buf: the reference's is_valid_number, so 1e4 itself and -1e30 are valid.
 *   counters  NULL, or two int32 in device memory: one thread of workgroup 0 adds 1 to counters[0] (step applied) or
 *             counters[1] (step skipped) with a plain load and store - launches are stream-ordered, no atomic.
 *   zero_grads != 0: every g the launch covers is overwritten with 0, whether the step was applied or skipped.
 * A launch writes p, buf (applied steps), g (zero_grads) and one counter, and nothing else; the table and the guard are only read. */
#define USOT_SGD_FIRST     1   /* flags bit 0: buf' = d (the tensor's first step; buf is not read) */
#define USOT_SGD_NESTEROV  2   /* flags bit 1 */
#define USOT_SGD_MAXIMIZE  4   /* flags bit 2 */
typedef struct usot_sgd_tensor {
    float *p;                       /* [n] parameter, updated in place */
    float *g;                       /* [n] gradient; zeroed with zero_grads, otherwise only read */
    float *buf;                     /* [n] momentum buffer, updated in place; NULL allowed with momentum == 0 */
    int64_t n;                      /* elements; 0 = the tensor takes no part */
    float lr, weight_decay, momentum, grad_scale;
    int32_t flags;                  /* USOT_SGD_* */
    int32_t reserved;               /* 0 in the image: three pointers, n, four floats and flags are 52 bytes, the record is 56 */
} usot_sgd_tensor;
typedef struct usot_sgd_launch {
    const void *table;              /* device address of the uploaded image */
    const float *guard;             /* device; NULL = no guard */
    int32_t *counters;              /* device, 2 x int32; NULL = not counted */
    int64_t n_chunks;               /* of the image (usot_sgd_table_bytes) */
    int32_t T;                      /* records in the image */
    int32_t zero_grads;
} usot_sgd_launch;
int     usot_sgd_chunk_elems(void);                                               /* host only: elements per chunk */
int     usot_sgd_grid_cap(void);                                                  /* host only: most workgroups of a launch */
int64_t usot_sgd_table_bytes(const int64_t *n, int T, int64_t *n_chunks);        /* host only */
int     usot_sgd_table_fill(const usot_sgd_tensor *t, int T, void *image, int64_t bytes);      /* host only */
int     usot_sgd_step_f32(void *stream, const usot_sgd_launch *d);

/* ---- fused GroupDW on NHWC (connect.py:86-102): three depthwise xcorrs and the
 * softmax(weight)-weighted sum in one pass, no intermediate maps.
 *   branch b: x_b NHWC [XS][OH+hk_b-1][OW+wk_b-1] (pixel stride x_cs, channel offset x_co)
 *             z_b NHWC [S][hk_b][wk_b]            (pixel stride z_cs, channel offset z_co)
 *   sample s uses search map s / x_rep (x_rep = N_q for the memory branch, where the
 *   reference materialises a 7x repeat, connect.py:258-264) and template s.
 *   out NHWC [S][OH][OW][C];  wsm = softmax(weight) (3 floats, host pointer).          */
typedef struct usot_groupdw_desc {
    const float *x[3];
    const float *z[3];
    float *out;
    int32_t hk[3], wk[3];
    int32_t x_cs[3], x_co[3], z_cs[3], z_co[3];
    float wsm[3];
    int32_t S, x_rep, OH, OW, C;
    int32_t cols_per_thread;     /* kernel variant, read from d[0]; every variant computes the same sums (tests/test_gpu_groupdw_sweep.py):
                                  *  0  auto: below 64 samples 1; from 64 samples up 7 for 25- and 27-wide responses when every
                                  *     segment has x_rep 1, 6 when one shares its maps, 4 for OW 21 .. 30, else 1
                                  *  1  5x1 strips (what a single frame runs; the only variant that takes a run-time count)
                                  *  5 / 50 / 52  5x5 patches at 4 / 1 / 2 waves per SIMD (register budgets)
                                  *  2  column threads, OH <= 32
                                  *  3  LDS row streaming, OW 21 .. 30; 16-byte loads of the search rows: every x[b] 16-byte
                                  *     aligned, x_cs and x_co multiples of 4
                                  *  4  ring (taps in LDS, rows streamed once), OW 21 .. 30
                                  *  6 / 7  LDS-DMA (loader waves feed row-sets to LDS, 7-column strip waves) with the default /
                                  *     the non-temporal load policy, OW 25 or 27; x aligned as for 3
                                  *  8 / 9  the persistent form of 6 / 7 (the resident workgroups walk the (sample, channel group)
                                  *     units), OW 25 or 27; x AND z aligned as for 3 (the taps are DMA pieces too)
                                  * 1, 2, 4, 5, 50, 52 load by dwords: any x_cs / x_co / z_cs / z_co; 3, 6, 7 any z_cs / z_co.
                                  * OH is free except for 2.  6, 7, 8, 9 give the same bits.
                                  * USOT_EINVAL, nothing launched and no output written: nseg outside 1 .. 3, OH or OW < 1, C not a
                                  * positive multiple of 64, S < 1, x_rep < 1, a NULL x / z / out, hk / wk other than 5x5, 3x5, 5x3,
                                  * a segment whose OH / OW / C differs from d[0]'s, any other code, a geometry or an alignment the
                                  * variant does not take */
} usot_groupdw_desc;
int usot_groupdw_f32(void *stream, const usot_groupdw_desc *d);
/* the cols_per_thread code the launcher resolves 0 (auto) to for this many samples (benchmarks name
 * the kernel they time with it) */
int usot_groupdw_auto_variant(int total_samples, int OW);
/* up to three segments of identical geometry (the cls, reg and memory GroupDWs of a frame)
 * in ONE launch */
int usot_groupdw_multi_f32(void *stream, const usot_groupdw_desc *d, int nseg);
/* ... with the OUTPUT maps stored as fp16 (out_dtype 1) or bf16 (2) — d[i].out then points to 16-bit elements; the same fp32
 * arithmetic, one rounding at the store (the batched mixed-precision heads of BASELINE configs[4] feed these maps to fp16
 * convolutions).  25- and 27-wide responses only. */
int usot_groupdw_multi_lp(void *stream, const usot_groupdw_desc *d, int nseg, int out_dtype);
/* usot_groupdw_multi_f32 with the number of live samples of its LAST segment read from DEVICE memory at run time: *last_count,
 * clamped to [0, d[nseg - 1].S].  The grid stays sized for d[nseg - 1].S; workgroups of the samples past the count leave at once,
 * their outputs keep their old contents.  The 5 x 1 strips kernel (what a single frame runs) only: USOT_EINVAL where another
 * variant would run.  last_count == NULL: the static launch. */
int usot_groupdw_multi_dyn_f32(void *stream, const usot_groupdw_desc *d, int nseg, const int32_t *last_count);
int usot_plan_add_groupdw_multi_dyn(void *plan, const usot_groupdw_desc *d, int nseg, const int32_t *last_count);

/* ---- Conf_Fusion reduction (connect.py:132-142): cv NHWC [B*M][P][2C] holding
 * conf = exp(clamp) in channels [0,C) and value in [C,2C) -> out [B][P][C] =
 * sum_m conf*value / sum_m conf.                                                       */
int usot_conf_fusion_reduce_f32(void *stream, const float *cv, float *out,
                                int B, int M, int P, int C);
int usot_conf_fusion_reduce_lp(void *stream, const void *cv, int in_dtype, void *out, int B, int M, int P, int C, int out_dtype);   /* cv fp32 (0) | fp16 (1) | bf16 (2); out fp16 (1) | bf16 (2) */
/* the fp32 reduction through a slot map in DEVICE memory: slot m reads map map[m] (int32[M], entries in [0, M)) of its batch
 * element's block of M maps.  The sums run over the M slots in slot order, exactly as the static kernel sums a tensor gathered by
 * `map` - no weighting by multiplicity.  map == NULL: usot_conf_fusion_reduce_f32. */
int usot_conf_fusion_reduce_map_f32(void *stream, const float *cv, float *out, int B, int M, int P, int C, const int32_t *map);
int usot_plan_add_conf_reduce_map(void *plan, const float *cv, float *out, int B, int M, int P, int C, const int32_t *map);

/* ---- Precise RoI Pooling forward.  Replaces PrRoIPoolingForwardGpu
 * (prroi_pooling_gpu_impl.cuh:20-28 / .cu:149-212,387-402) with explicit strides so the
 * same kernel reads NCHW (API edge) or NHWC (engine) features and writes either layout.
 *   feat element (b,c,h,w) at b*f_sb + c*f_sc + h*f_sh + w*f_sw
 *   rois [R][5] = (batch, x1, y1, x2, y2);  out element (r,c,ph,pw) at
 *   r*o_sr + c*o_sc + ph*o_sh + pw*o_sw                                                */
int usot_prroi_pool_forward_f32(void *stream, const float *feat, const float *rois, float *out,
                                int R, int C, int H, int W, int PH, int PW, float scale,
                                int64_t f_sb, int64_t f_sc, int64_t f_sh, int64_t f_sw,
                                int64_t o_sr, int64_t o_sc, int64_t o_sh, int64_t o_sw);

/* ---- the reference's native symbol, with the reference's signature
 * (lib/models/prroi_pool/src/prroi_pooling_gpu_impl.cuh:20-28; launcher .cu:387-402): contiguous
 * NCHW float32 features, rois [R][5], contiguous [R][C][PH][PW] output, top_count = R*C*PH*PW,
 * enqueued on `stream`.  prroi_pooling_gpu.c:22-44 links against it unchanged.
 * A shim over usot_prroi_pool_forward_f32; on a bad argument or a failed launch it prints one line
 * to stderr and returns — it does not exit(-1) as the reference's launcher does
 * (prroi_pooling_gpu_impl.cu:20-27).                                                          */
typedef struct ihipStream_t *hipStream_t;      /* identical to <hip/hip_runtime_api.h>'s typedef */
void PrRoIPoolingForwardGpu(hipStream_t stream, const float *bottom_data, const float *bottom_rois,
                            float *top_data, const int channels_, const int height_, const int width_,
                            const int pooled_height_, const int pooled_width_,
                            const float spatial_scale_, const int top_count);

/* ---- gradients of Precise RoI Pooling: what the reference's binding exposes for training
 * (prroi_pooling_gpu.c:46-113).  Contiguous NCHW features [B][C][H][W], rois [R][5], top_data / top_diff
 * [R][C][PH][PW].  Both zero-fill their output on the stream first (as .cu:415,436).
 *   backward:       bottom_diff [B][C][H][W] += top_diff / bin area * (weight of the pixel in the bin integral)
 *   coor_backward:  rois_diff [R][5] = d sum(top_diff * out) / d (batch, x1, y1, x2, y2); column 0 is 0.
 *                   A RoI whose batch index is outside [0, B) contributes nothing.                              */
int usot_prroi_pool_backward_f32(void *stream, const float *rois, const float *top_diff, float *bottom_diff,
                                 int R, int B, int C, int H, int W, int PH, int PW, float scale);
int usot_prroi_pool_coor_backward_f32(void *stream, const float *feat, const float *rois, const float *top_data,
                                      const float *top_diff, float *rois_diff,
                                      int R, int B, int C, int H, int W, int PH, int PW, float scale);

/* the reference's symbols for them, exact signatures (prroi_pooling_gpu_impl.cuh:30-54; launchers .cu:404-440);
 * on a bad argument or a failed launch: one line on stderr and return, never exit(-1) */
void PrRoIPoolingBackwardGpu(hipStream_t stream, const float *bottom_data, const float *bottom_rois,
                             const float *top_data, const float *top_diff, float *bottom_diff,
                             const int channels_, const int height_, const int width_,
                             const int pooled_height_, const int pooled_width_, const float spatial_scale_,
                             const int top_count, const int bottom_count);
void PrRoIPoolingCoorBackwardGpu(hipStream_t stream, const float *bottom_data, const float *bottom_rois,
                                 const float *top_data, const float *top_diff, float *bottom_diff,
                                 const int channels_, const int height_, const int width_,
                                 const int pooled_height_, const int pooled_width_, const float spatial_scale_,
                                 const int top_count, const int bottom_count);

/* ---- layout changes at the API edge: generic 4-D strided copy ----------------------
 * dst[n][a][b][c] (dense) = src[n*s0 + a*s1 + b*s2 + c*s3]                              */
int usot_permute4_f32(void *stream, const float *src, float *dst,
                      int D0, int D1, int D2, int D3,
                      int64_t s0, int64_t s1, int64_t s2, int64_t s3);

/* ---- on-device decode of one frame (usot_tracker.py:138-163): float32 sigmoid and
 * offline/online blend, then (in float64, as numpy promotes there because the grids are
 * float64) box decode, size/ratio penalty, cosine window and first-max argmax.
 * cls/cls_mem [S*S] logits, bbox [4][S*S], window [S*S] float64;
 * out[8] = {best_index, blended_score, penalty, x1, y1, x2, y2, pscore} (float64).
 * tw/th = target size already multiplied by scale_z (usot_tracker.py:258).              */
int usot_decode_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox,
                    const double *window, double *out, int S, int instance_size, int stride,
                    float ratio, double penalty_k, double window_influence,
                    double tw, double th);

/* same, with the target size read from device memory (double[2]) and, if roi_out != NULL,
 * the PrRoIPool box of the winning cell (usot_tracker.py:196, 329-350) written to
 * roi_out[5] = (0, x1, y1, x2, y2) in feature coordinates: no host round trip between
 * decode and memory-feature pooling.  tsz_dev[6] is a caller-chosen frame tag that is copied
 * to out[8] AFTER the results (system-scope fence in between), so `out` needs 9 doubles and a
 * host may poll out[8] in pinned memory instead of synchronising the stream.
 * tsz_dev[3], read as a 64-bit integer: 0, or the device address of the frame's sticky split-fp16 range word
 * (usot_conv_desc.ovf); its value is then published as out[9] (10 doubles) with the results and the word is cleared. */
int usot_decode_dev_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox,
                        const double *window, double *out, int S, int instance_size, int stride,
                        float ratio, double penalty_k, double window_influence,
                        const double *tsz_dev, float *roi_out);

/* ---- SiamFC crop on the device (lib/utils/track_utils.py:30-119, get_subwindow_tracking):
 * window [x0, x0+win) x [y0, y0+win) of an HWC uint8 BGR frame (coordinates may leave the
 * image: mean-colour fill, values already truncated to uint8 like numpy's assignment),
 * OpenCV-style fixed-point bilinear resize to S x S when win != S, CHW float32 output.     */
int usot_crop_resize_u8_f32(void *stream, const unsigned char *im, float *out, int H, int W,
                            int x0, int y0, int win, int S, int fill_b, int fill_g, int fill_r);

/* ---- row gather (scatter = 0: dst[i] = src[idx[i]]) / scatter (dst[idx[i]] = src[i]) of
 * `n_rows` rows of `row_len` floats with indices read from DEVICE memory: selects the
 * memory-queue kernels of a frame (usot_tracker.py:222-256) and appends the new one
 * (:264) inside a captured graph.                                                        */
int usot_rows_copy_f32(void *stream, const float *src, const int32_t *idx_dev, float *dst,
                       int n_rows, int row_len, int scatter);

/* ---- launch plans: record the per-frame kernel sequence once, replay it natively, or
 * capture it into a hipGraph (one hipGraphLaunch per frame).  Pointers are baked at add
 * time, so they must refer to buffers that outlive the plan (the engine's workspace).
 * fork(lane>0): that lane waits for lane 0, following ops go to `lane`; fork(0): back to
 * lane 0 without waiting; join(lane): lane 0 waits for `lane`.  Lanes are extra streams
 * (parallel graph branches after capture); run() on an uncaptured plan ignores lanes and
 * issues everything in program order on the caller's stream.                             */
void *usot_plan_create(void);
void usot_plan_destroy(void *plan);
int usot_plan_size(void *plan);
int usot_plan_add_conv(void *plan, const usot_conv_desc *d);
int usot_plan_add_conv_batch(void *plan, const usot_conv_desc *d, int n);
int usot_plan_add_conv_bf16(void *plan, const usot_conv_desc *d);
int usot_plan_add_conv_lp(void *plan, const usot_conv_desc *d, int dtype, int out_f32);
int usot_plan_add_cvt_lp(void *plan, const float *src, void *dst, int64_t n, int dtype);
int usot_plan_add_maxpool_lp(void *plan, const void *x, void *y, int N, int H, int W, int C, int OH, int OW, int dtype);
int usot_plan_add_stem_pool_lp(void *plan, const float *x, const void *wfrag, const float *bias, void *y,
                               int N, int H, int W, int OH, int OW, int PH, int PW, int dtype,
                      float mu0, float mu1, float mu2);
int usot_plan_add_cvt_bf16(void *plan, const float *src, void *dst, int64_t n);
int usot_plan_add_maxpool_bf16(void *plan, const void *x, void *y, int N, int H, int W, int C, int OH, int OW);
int usot_plan_add_groupdw(void *plan, const usot_groupdw_desc *d);
int usot_plan_add_groupdw_multi(void *plan, const usot_groupdw_desc *d, int nseg);
int usot_plan_add_groupdw_multi_lp(void *plan, const usot_groupdw_desc *d, int nseg, int out_dtype);
/* fused fp32 stem + max-pool on the fp32 MFMA (the 125x125 stem map never reaches HBM); wfrag from
 * usot_amd/engine.py: pack_stem_f32 */
int usot_stem_pool_f32(void *stream, const float *x, const float *wfrag, const float *bias, float *y,
                       int N, int H, int W, int OH, int OW, int PH, int PW);
int usot_plan_add_stem_pool(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                            int N, int H, int W, int OH, int OW, int PH, int PW);
/* the same with the crop's address taken from DEVICE memory at run time: xptr_dev[0..1] = low / high half of the
 * address (0 = use x).  A captured frame can then read any resident crop without a copy into a baked input
 * buffer; the session's first kernel stashes the address there from the host's control block. */
int usot_stem_pool_ind_f32(void *stream, const float *x, const float *wfrag, const float *bias, float *y,
                           int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev);
int usot_plan_add_stem_pool_ind(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                                int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev);
int usot_plan_add_stem(void *plan, const float *x, const float *w, const float *bias, float *y,
                       int N, int H, int W, int OH, int OW);
/* ... and both stem forms on x - mu[ci] (see usot_stem_conv_mu_f32) */
int usot_stem_pool_mu_f32(void *stream, const float *x, const float *wfrag, const float *bias, float *y,
                          int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev,
                          float mu0, float mu1, float mu2);
int usot_plan_add_stem_pool_mu(void *plan, const float *x, const float *wfrag, const float *bias, float *y,
                               int N, int H, int W, int OH, int OW, int PH, int PW, const int32_t *xptr_dev,
                               float mu0, float mu1, float mu2);
int usot_plan_add_stem_mu(void *plan, const float *x, const float *w, const float *bias, float *y,
                          int N, int H, int W, int OH, int OW, float mu0, float mu1, float mu2);
int usot_plan_add_maxpool(void *plan, const float *x, float *y, int N, int H, int W, int C,
                          int OH, int OW);
int usot_plan_add_conf_reduce(void *plan, const float *cv, float *out, int B, int M, int P, int C);
int usot_plan_add_conf_reduce_lp(void *plan, const void *cv, int in_dtype, void *out, int B, int M, int P, int C, int out_dtype);
int usot_plan_add_prroi(void *plan, const float *feat, const float *rois, float *out,
                        int R, int C, int H, int W, int PH, int PW, float scale,
                        int64_t f_sb, int64_t f_sc, int64_t f_sh, int64_t f_sw,
                        int64_t o_sr, int64_t o_sc, int64_t o_sh, int64_t o_sw);
int usot_plan_add_permute(void *plan, const float *src, float *dst, int D0, int D1, int D2, int D3,
                          int64_t s0, int64_t s1, int64_t s2, int64_t s3);
int usot_plan_add_decode(void *plan, const float *cls, const float *cls_mem, const float *bbox,
                         const double *window, double *out, int S, int instance_size, int stride,
                         float ratio, double penalty_k, double window_influence,
                         const double *tsz_dev, float *roi_out);
/* the same for up to four banks of different row length (one launch): the session's raw memory
 * features and their three cached encodings share the row indices.  stash_next (gather only, may
 * be NULL): idx_dev[n_rows .. n_rows+2] are copied to stash_next[0..2] (the append row, and two free words the
 * session uses for the crop address of usot_plan_add_stem_pool_ind), so that a later scatter of the same frame
 * can take its row from device memory while the host already rewrites the control block. */
int usot_rows_copy_multi_f32(void *stream, int nseg, const float *const *src, const int32_t *idx_dev,
                             float *const *dst, int n_rows, const int32_t *row_len, int scatter,
                             int32_t *stash_next);
int usot_plan_add_rows_copy_multi(void *plan, int nseg, const float *const *src, const int32_t *idx_dev,
                                  float *const *dst, int n_rows, const int32_t *row_len, int scatter,
                             int32_t *stash_next);
/* append + gather in one launch (the session's 'defer_append' = 2 frame): fresh[0..3] = the memory feature the previous frame
 * pooled and its three kernel-side encodings (one row each), bank[0..3] their banks, picked[0..2] the frame's picked-kernel
 * buffers of banks 1-3 (n_pick <= 32 rows each).  Row idx_dev[slot_pos] of every bank receives the fresh row, rows
 * idx_dev[0 .. n_pick) of banks 1-3 are gathered - one that IS the appended row is taken from `fresh`.  idx_dev may be pinned
 * host memory (the control block).  Replaces usot_rows_copy_multi_f32 (scatter) + usot_rows_copy_multi_f32 (gather);
 * the reference keeps the queue in Python lists (usot_tracker.py:222-264). */
int usot_rows_append_gather_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos);
int usot_plan_add_rows_append_gather(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                     const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos);
/* the same launch on DISTINCT picked rows only.  With first(j) = the smallest i <= j whose row equals row j and u(j) = the rank of
 * first(j) among first occurrences (distinct rows keep their order of first appearance, D of them), only rows j == first(j) are
 * copied, to picked[g][u(j)]; rows >= D of the picked buffers are NOT written.  mem_map (DEVICE memory, int32[1 + n_pick]) receives
 * mem_map[0] = D and mem_map[1 + j] = u(j): the sample count, image count and slot map of the launches behind it
 * (usot_groupdw_multi_dyn_f32, usot_conv_desc.n_dyn, usot_conf_fusion_reduce_map_f32).  The append half and the "a picked row that
 * is the appended row comes from `fresh`" rule are unchanged. */
int usot_rows_append_gather_dedupe_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                       const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos, int32_t *mem_map);
int usot_plan_add_rows_append_gather_dedupe(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                            const int32_t *row_len, const int32_t *idx_dev, int n_pick, int slot_pos, int32_t *mem_map);
/* ---- lock-step multi-video tracking (csrc/multitrack.hip): B videos ("slots") of one instance size step together in one
 * frame graph.  Each kernel is ONE launch per step whatever B.  The step's control block `ctl` (pinned, device-mapped host
 * memory, or device memory) is a USOT_STEP_HDR_BYTES header - the step tag, a double, at offset 0 - followed by B
 * usot_slot_rec records.  Every kernel fetches the words of its slot once per workgroup, and every word is read before the
 * decode publishes the slot's tag, so the host may rewrite the block as soon as all B tags are seen.
 * Memory banks: one tensor per bank kind, [B * cap, row]; slot b's row r is global row b * cap + r. */
#define USOT_STEP_HDR_BYTES 64
typedef struct usot_slot_rec {
    double tsz[2];            /* target size x scale_z (decode)                                                      */
    uint64_t im;              /* device address of the slot's HWC uint8 image; 0 = the crop is not written (the host   */
                              /* wrote it, or the slot is inactive)                                                  */
    int32_t H, W;             /* image size                                                                          */
    int32_t x0, y0, win;      /* crop window: origin in image coordinates (may be negative) and edge                 */
    int32_t fill[3];          /* padding colour, B G R                                                               */
    int32_t append_row;       /* global bank row that receives the PREVIOUS step's pooled feature (a scratch row when */
                              /* nothing is pending)                                                                 */
    int32_t next_row;         /* global row this step's feature is appended to by the next step (host bookkeeping)   */
    int32_t picks[32];        /* N_q global bank rows gathered for this step's memory kernels                        */
} usot_slot_rec;              /* 192 bytes */
/* decode of B slots (one workgroup each, S <= 32): maps cls / cls_mem [B][S][S], bbox [B][4][S][S]; window [S][S] shared.
 * out: B rows of 16 doubles, row b = usot_decode_dev_f32's results [0..8) and the step tag at [8], stored after the results
 * behind a system-scope fence.  roi_out: B rows of 5 floats, (b, pool_label_search(box)) - the batch index is the slot. */
int usot_decode_batch_f32(void *stream, const float *cls, const float *cls_mem, const float *bbox, const double *window,
                          double *out, int B, int S, int instance_size, int stride, float ratio, double penalty_k,
                          double window_influence, const void *ctl, float *roi_out);
int usot_plan_add_decode_batch(void *plan, const float *cls, const float *cls_mem, const float *bbox, const double *window,
                               double *out, int B, int S, int instance_size, int stride, float ratio, double penalty_k,
                               double window_influence, const void *ctl, float *roi_out);
/* append + gather of B slots: fresh[k] [B][row_len[k]] (the previous step's pooled feature and its three encodings), bank[k]
 * [B * cap][row_len[k]], picked[k - 1] [B * n_pick][row_len[k]] (k = 1..3).  Slot b: fresh row b -> bank row append_row;
 * picks[j] -> picked row b * n_pick + j, a pick equal to append_row read from fresh row b.  n_pick <= 32.  bank_rows = B * cap:
 * a row outside [0, bank_rows) is never touched (such an append is dropped, such a pick gathers zeros). */
int usot_rows_append_gather_batch_f32(void *stream, const float *const *fresh, float *const *bank, float *const *picked,
                                      const int32_t *row_len, const void *ctl, int B, int n_pick, int bank_rows);
int usot_plan_add_rows_append_gather_batch(void *plan, const float *const *fresh, float *const *bank, float *const *picked,
                                           const int32_t *row_len, const void *ctl, int B, int n_pick, int bank_rows);
/* crop + resize of B slots into out [B][3][S][S]: slot b's window from its record, usot_crop_resize_u8_f32's arithmetic;
 * a slot whose image address is 0 is left untouched. */
int usot_crop_resize_batch_u8_f32(void *stream, const void *ctl, float *out, int B, int S);
int usot_plan_add_crop_resize_batch(void *plan, const void *ctl, float *out, int B, int S);
int usot_plan_add_rows_copy(void *plan, const float *src, const int32_t *idx_dev, float *dst,
                            int n_rows, int row_len, int scatter);
int usot_plan_fork(void *plan, int lane);
int usot_plan_join(void *plan, int lane);
int usot_plan_capture(void *plan, void *stream);
int usot_plan_run(void *plan, void *stream);
/* per-op mean milliseconds per launch (HIP events on `stream`, eager, program order, each op
 * launched `reps` times between its two events), blocking */
int usot_plan_profile(void *plan, void *stream, int frames, int reps, float *ms_per_op);
/* info[4] = {kind, conv tile id, ksplit, groups} of op i.  tile: kind 0 - the tile the launcher would pick NOW
 * (usot_conv_resolve_tile on the first descriptor), kind 11 - the descriptor's tile field, else 0; ksplit / groups: kind 0 (first
 * descriptor), else 1.  The kinds - an op's kind names its ADDER, the entry point it launches is listed behind it.  The numbers
 * are FROZEN: bench.py, the tests and the scripts match on them; a new kind takes the next free number.
 *    0  conv, conv_batch          usot_conv2d_f32 (one problem) | usot_conv2d_batch_f32
 *    1  stem, stem_mu             usot_stem_conv_mu_f32
 *    2  maxpool                   usot_maxpool3x3s2_f32
 *    3  groupdw, groupdw_multi, groupdw_multi_dyn   usot_groupdw_multi_dyn_f32;  groupdw_multi_lp   usot_groupdw_multi_lp
 *    4  conf_reduce, conf_reduce_map   usot_conf_fusion_reduce_map_f32;  conf_reduce_lp   usot_conf_fusion_reduce_lp
 *    5  prroi                     usot_prroi_pool_forward_f32
 *    6  permute                   usot_permute4_f32
 *    7  decode                    usot_decode_dev_f32
 *    8  fork                      (no launch: the lane waits for lane 0)
 *    9  join                      (no launch: lane 0 waits for the lane)
 *   10  rows_copy                 usot_rows_copy_f32
 *   11  conv_lp, conv_bf16        usot_conv2d_lp
 *   12  cvt_lp, cvt_bf16          usot_cvt_f32_to_lp
 *   13  maxpool_lp, maxpool_bf16  usot_maxpool3x3s2_lp
 *   14  stem_pool_lp              usot_stem_pool_lp
 *   15  rows_copy_multi           usot_rows_copy_multi_f32
 *   16  thin_conv                 usot_thin_conv3x3_f32
 *   17  stem_pool, stem_pool_ind, stem_pool_mu   usot_stem_pool_mu_f32
 *   18  pw_pair                   usot_pw_pair_lp (dtype 0 | 1) | usot_pw_pair_f32 (2) | usot_pw_pair_f32s (3)
 *   19  pw_single                 usot_pw_single_f32
 *   20  stream_conv3x3            usot_stream_conv3x3_f32
 *   21  pw_triple                 usot_pw_triple_f32
 *   22  pw_panel                  usot_pw_panel_lp
 *   23  pw_panel_pair             usot_pw_panel_pair_lp
 *   24  conv3x3_halo              usot_conv3x3_halo_lp
 *   25  pw_kstream                usot_pw_kstream_lp
 *   26  conv_kstream              usot_conv_kstream_lp
 *   27  bneck_first               usot_bneck_first_lp
 *   28  bneck_tail                usot_bneck_tail_lp
 *   29  conv_pw                   usot_conv_pw_lp
 *   30  conv_pw_pair              usot_conv_pw_pair_lp
 *   31  conv_pw_ov                usot_conv_pw_ov_lp
 *   32  rows_append_gather        usot_rows_append_gather_f32;  rows_append_gather_dedupe   usot_rows_append_gather_dedupe_f32
 *   33  decode_batch              usot_decode_batch_f32
 *   34  rows_append_gather_batch  usot_rows_append_gather_batch_f32
 *   35  crop_resize_batch         usot_crop_resize_batch_u8_f32 */
int usot_plan_op_info(void *plan, int i, int *info);
int usot_conv_resolve_tile(const usot_conv_desc *d);

#ifdef __cplusplus
}
#endif
#endif /* USOT_HIP_H */
