/* sntc.h -- C ABI of the MI355X-native shallow-ntc hot path (libsntc_hip.so).
 *
 * The reference (mandt-lab/shallow-ntc) has no FFI: its arithmetic is TensorFlow /
 * tensorflow-compression ops called from Python.  Each entry point below replaces ONE of those
 * dependency ops at the place the reference calls it; the citations are reference file:line.
 * INTEGRATION.md shows the ctypes binding a maintainer would add to the reference.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types cross the boundary.
 *   - every function returns an int status (SNTC_OK == 0); sntc_last_error() gives the
 *     thread-local message of the last failure.  No exceptions cross the boundary.
 *   - all tensor pointers are DEVICE pointers to dense NHWC float32 unless stated; the caller
 *     owns every buffer.  The library owns only what a plan / prior object packs at creation.
 *   - every launch takes a hipStream_t (passed as void*) and is asynchronous w.r.t. the host.
 *   - one process per GPU; objects are bound to the device current at creation.
 */
#ifndef SNTC_H_
#define SNTC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNTC_VERSION 100

/* status codes (mirroring the failure classes of the reference: Python ValueError for shapes /
 * configs, tf InvalidArgumentError from check_numerics at mshyper/models.py:308-309,356) */
enum {
  SNTC_OK = 0,
  SNTC_ERR_BAD_SHAPE = 1,      /* inconsistent sizes / null pointer                           */
  SNTC_ERR_UNSUPPORTED = 2,    /* configuration outside what the kernels implement            */
  SNTC_ERR_HIP = 3,            /* HIP runtime error (message carries hipGetErrorString)       */
  SNTC_ERR_NONFINITE = 4,      /* NaN/Inf where the reference's check_numerics would raise    */
  SNTC_ERR_NO_DEVICE = 5       /* no gfx950 device visible                                    */
};

const char* sntc_last_error(void);
int sntc_version(void);
/* Number of visible HIP devices, 0 if none; never fails. */
int sntc_device_count(void);
/* Writes the gcnArchName of `device` ("gfx950:sramecc+:xnack-") into buf. */
int sntc_device_arch(int device, char* buf, size_t buflen);

/* ------------------------------------------------------------------------------------------
 * Convolution plans
 *   replaces tf.keras.layers.Conv2D / Conv2DTranspose (padding="SAME") and tfc.SignalConv2D
 *   (padding="same_zeros") at common/transforms.py:81-90,101-134,152-155,172-175,186-231,
 *   240-262,284-287,307-313,331-357,371-373 and common/elic.py:61-63,92-93,136-140,253-270;
 *   and the 1x1 norm-pool contraction of GDN / GDN1 at common/transforms.py:8-63,150,170.
 * ------------------------------------------------------------------------------------------ */
enum {                       /* sntc_conv_desc.kind */
  SNTC_CONV2D = 0,           /* Keras Conv2D SAME, kernel [kh,kw,Cin,Cout], cross-correlation */
  SNTC_CONV2D_TRANSPOSE = 1, /* Keras Conv2DTranspose SAME, kernel [kh,kw,Cout,Cin]           */
  SNTC_SIGNAL_DOWN = 2,      /* tfc.SignalConv2D corr=True, strides_down, same_zeros, [kh,kw,Cin,Cout] */
  SNTC_SIGNAL_UP = 3         /* tfc.SignalConv2D corr=False, strides_up, same_zeros, [kh,kw,Cin,Cout]  */
};
enum {                       /* activation applied after bias (Keras `activation=`) */
  SNTC_ACT_NONE = 0, SNTC_ACT_RELU = 1, SNTC_ACT_LEAKY_RELU = 2 /* alpha 0.2 */, SNTC_ACT_SIGMOID = 3
};
enum {                       /* input transform applied to x while it is staged (GDN norm pool) */
  SNTC_PRO_NONE = 0, SNTC_PRO_ABS = 1, SNTC_PRO_SQUARE = 2
};
enum {                       /* epilogue, v = act(conv + bias) */
  SNTC_EPI_STORE = 0,        /* y = v                                                          */
  SNTC_EPI_ADD = 1,          /* y = v + res                (ResidualBlock skip, elic.py:66-68)  */
  SNTC_EPI_GATE = 2,         /* y = res + aux * v          (SimpleAttention, elic.py:97-100)    */
  SNTC_EPI_RES_DIV = 3,      /* y = res / v                (GDN1 forward, transforms.py:63)     */
  SNTC_EPI_RES_MUL = 4,      /* y = res * v                (GDN1 inverse, transforms.py:61)     */
  SNTC_EPI_RES_DIV_SQRT = 5, /* y = res / sqrt(v)          (classic tfc.GDN)                    */
  SNTC_EPI_RES_MUL_SQRT = 6, /* y = res * sqrt(v)          (classic inverse tfc.GDN)            */
  SNTC_EPI_MASK_RELU = 7,    /* y = res > 0 ? v : 0        (relu backward; res = forward output) */
  SNTC_EPI_MASK_LEAKY = 8,   /* y = res >= 0 ? v : 0.2 v   (leaky-relu backward)                 */
  SNTC_EPI_DEQUANT = 9       /* y = v + (float)s, s int32  (decoder: y_hat = symbols + mu, mshyper/models.py:278-279).  A per-call
                              * override of a SNTC_EPI_STORE plan (sntc_conv_forward_columns_dequant), never a plan's own epilogue */
};

typedef struct sntc_conv_desc {
  int32_t kind;        /* SNTC_CONV2D ...                                  */
  int32_t kh, kw;      /* kernel size                                      */
  int32_t stride;      /* strides (down for conv, up for transpose)        */
  int32_t cin, cout;   /* channels                                         */
  int32_t act;         /* SNTC_ACT_*                                       */
  int32_t prologue;    /* SNTC_PRO_*                                       */
  int32_t epilogue;    /* SNTC_EPI_*                                       */
  int32_t reserved[7]; /* reserved[0] != 0: the kernel array has its two channel axes swapped with respect to the kind's
                        * native layout (so that the input-gradient plan of a layer -- the adjoint kind -- packs straight
                        * from the layer's own kernel array; Keras Conv2D <-> Conv2DTranspose are each other's swap already,
                        * tfc.SignalConv2D down <-> up need the flag);
                        * reserved[1] != 0: bf16 x 3 split-precision contraction (hi + mid + lo bfloat16 terms, six cross
                        * products on the bf16 matrix cores, fp32 accumulation): ~1e-7 relative like fp32 but NOT
                        * bit-identical to it; Cin % 16 == 0, no prologue; opt-in (Model(precision="bf16x3")), never a default.
                        *   1: fp32 NHWC input, split while it is staged (the round-2 experiment);
                        *   2: the INPUT is pre-split too -- format S3, see sntc_split3 -- and the launch runs the 256-wide
                        *      direct-to-LDS kernel of csrc/bf3_gemm.hip; output fp32 NHWC; Cout % 4 == 0, epilogues
                        *      STORE / ADD / GATE / MASK_*; no split-K;
                        * reserved[2] == 1: ROW-PACKED small-Cin convolution (the RGB first layer: Keras Conv2D 5x5 / 2, Cin = 3,
                        *   common/elic.py:147, common/transforms.py:183): kw * Cin <= 16, fp32, no prologue.  The caller applies
                        *   the SAME padding itself (sntc_pad_zero) and the plan convolves VALID on that tensor: every kernel row
                        *   is one 16-deep K stage whose 64-B activation slab is ONE contiguous 16-B-per-lane read starting at
                        *   the window's first pixel -- the vector loader of the wide layers instead of 75 dword gathers per
                        *   output; out size = (padded - k) / stride + 1;
                        * the rest must be 0 */
} sntc_conv_desc;

typedef struct sntc_conv_plan sntc_conv_plan;

/* Packs `weight` (device pointer, layout per desc.kind) and `bias` (device [cout] or NULL) into
 * the gather-GEMM layout on `stream`.  The plan keeps its own packed copy; weight/bias may be
 * freed after the stream work completes. */
int sntc_conv_plan_create(const sntc_conv_desc* desc, const float* weight, const float* bias,
                          void* stream, sntc_conv_plan** plan);
void sntc_conv_plan_destroy(sntc_conv_plan* plan);
/* Re-pack an existing plan from new device weights (and bias: present iff the plan has one); tables and tile
 * choices are kept.  The training step calls this after every optimizer update. */
int sntc_conv_plan_update(sntc_conv_plan* plan, const float* weight, const float* bias, void* stream);
/* Every plan of a model re-packed by ONE launch: the training step (reference common/train_lib.py:185-215, one
 * optimizer.apply_gradients per step over all variables) changes every kernel at once, and ~170 plans x (pack + bias copy)
 * is ~400 tiny launches otherwise.  The group remembers, per plan, the device arrays its weights (and bias; NULL iff the
 * plan has none) are read from -- views of the trainer's flat variable store, which never move -- and
 * sntc_plan_group_update() does what sntc_conv_plan_update() would do for each of them, bit for bit.  The plans must
 * outlive the group. */
typedef struct sntc_plan_group sntc_plan_group;
int sntc_plan_group_create(sntc_conv_plan* const* plans, const float* const* weights, const float* const* biases, int count,
                           void* stream, sntc_plan_group** group);
int sntc_plan_group_update(const sntc_plan_group* group, void* stream);
void sntc_plan_group_destroy(sntc_plan_group* group);
/* Output spatial size for an input of h x w. */
int sntc_conv_out_shape(const sntc_conv_plan* plan, int h, int w, int* ho, int* wo);
/* Algorithmic 2*MAC FLOPs of one forward call (dense count, as tf.profiler counts them). */
int64_t sntc_conv_flops(const sntc_conv_plan* plan, int n, int h, int w);
/* y[n,ho,wo,cout] = epilogue(act(conv(prologue(x[n,h,w,cin])) + bias), res, aux).
 * res / aux are NHWC tensors of the OUTPUT shape (NULL unless the epilogue uses them). */
int sntc_conv_forward(const sntc_conv_plan* plan, const float* x, int n, int h, int w, float* y,
                      const float* res, const float* aux, void* workspace, size_t workspace_bytes, void* stream);
/* Device scratch the call above needs.  Large launches run on persistent stream-K workers that hand a tile's
 * accumulators to the next worker through this scratch (a few tens of MB, contents irrelevant before and after the call).
 * Layers that offer few output tiles per image but a long contraction (hyper transforms, SGA input-gradient
 * convolutions) are split along K into slabs that a second kernel adds in a fixed order; the split depends on the
 * layer and the image shape only.  Either way results are bit-identical for any batch size. */
int64_t sntc_conv_workspace_bytes(const sntc_conv_plan* plan, int n, int h, int w);
/* The tail of a ResidualBlock (reference common/elic.py:57-68: conv3x3(c/2 -> c/2, relu) -> conv1x1(c/2 -> c), + x) in ONE
 * launch for c = 192: `first` is the 3x3 plan (stride-1 forward convolution, 96 output channels, plain store), `second` the
 * 1x1 plan 96 -> 192 (no activation; its epilogue -- SNTC_EPI_ADD for the skip -- and `res` / `aux` apply to the final output
 * y[n,ho,wo,192]).  The 96-channel intermediate stays in registers; the result is bit-identical to sntc_conv_forward(first)
 * followed by sntc_conv_forward(second).  sntc_conv_fusable() says whether a pair qualifies (1) or not (0);
 * sntc_conv_fused_workspace_bytes() is the scratch this call needs (as sntc_conv_workspace_bytes). */
int sntc_conv_fusable(const sntc_conv_plan* first, const sntc_conv_plan* second);
int64_t sntc_conv_fused_workspace_bytes(const sntc_conv_plan* first, int n, int h, int w);
int sntc_conv_forward_fused(const sntc_conv_plan* first, const sntc_conv_plan* second, const float* x, int n, int h, int w, float* y,
                            const float* res, const float* aux, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------------------------------
 * The whole ResidualBlock (reference common/elic.py:41-68; inside SimpleAttention :85-100 and ElicAnalysis :147-163) in
 * ONE launch:  y = x + conv1x1_{c/2 -> c}( relu(conv3x3_{c/2 -> c/2}( relu(conv1x1_{c -> c/2}(x)) )) ),  NHWC fp32.
 * A workgroup owns an 8 x 32 pixel tile: the 1x1 head is computed on the tile's 10 x 34 halo patch straight into LDS
 * (out-of-image patch pixels = the 3x3's SAME zero padding), the 3x3's nine taps are nine shifted reads of that patch, and
 * its accumulators feed the 1x1 tail + skip from the registers -- neither c/2-channel intermediate touches HBM.  Every
 * output is the same k-ordered fp32 fma chain as in the three sntc_conv_forward launches: bit-identical to them, for any
 * batch size and any number of workgroups.
 *   w0 [1,1,c,c/2], w1 [3,3,c/2,c/2], w2 [1,1,c/2,c]: the Keras HWIO kernels (device pointers); b0, b1, b2: biases or NULL.
 * sntc_resblock_supported(c): 1 where the kernel exists (c = 192), else 0 -- callers then run the three layers.
 * x and y must not alias (tiles read their neighbours' halo); n*h*w*c*4 < 2 GiB per call.
 * precision 0: exact fp32 (the above).  precision 1: the same kernel structure in bf16 x 3 split precision (three bfloat16
 * terms per fp32 operand, six cross products on v_mfma_f32_32x32x16_bf16, fp32 accumulate; weights pre-split at plan creation,
 * pixels split in registers; x and y stay fp32 NHWC): fp32-level accuracy against float64, NOT bit-identical to precision 0 --
 * what Model(precision="bf16x3") runs, batch-invariant like everything else. */
typedef struct sntc_resblock_plan sntc_resblock_plan;
int sntc_resblock_supported(int c);
int sntc_resblock_plan_create(int c, const float* w0, const float* b0, const float* w1, const float* b1,
                              const float* w2, const float* b2, int precision, void* stream, sntc_resblock_plan** plan);
int sntc_resblock_plan_update(sntc_resblock_plan* plan, const float* w0, const float* b0, const float* w1, const float* b1,
                              const float* w2, const float* b2, void* stream);
void sntc_resblock_plan_destroy(sntc_resblock_plan* plan);
/* Algorithmic 2*MAC FLOPs of one call: 2 n h w (c c/2 + 9 (c/2)^2 + c/2 c), the three layers' sntc_conv_flops. */
int64_t sntc_resblock_flops(const sntc_resblock_plan* plan, int n, int h, int w);
int sntc_resblock_forward(const sntc_resblock_plan* plan, const float* x, int n, int h, int w, float* y, void* stream);
/* Cap the persistent workgroups of THIS plan's launches (0 = one per CU): tests assert that results do not depend on it. */
int sntc_resblock_plan_set_workgroups(sntc_resblock_plan* plan, int max_workgroups);
/* ------------------------------------------------------------------------------------------
 * The RGB first layer of the analysis transforms (reference common/elic.py:147 through build_conv :253-270 -- Keras
 * Conv2D(channels[0], 5, strides=2, padding="SAME") on the 3-channel image; common/transforms.py:183 CNNAnalysis' first layer) as
 * ONE launch of a kernel of its own:  y[n, ceil(h/2), ceil(w/2), cout] = act(conv(x) + bias),  x [n, h, w, 3] NHWC fp32.
 * A persistent workgroup owns 8 x 32 output pixels at a time (wave = tile row, lane = pixel, registers = all cout channels); the
 * packed weights stay in LDS, the tile's 19-row input patch is double-buffered there (SAME padding = zeros in the patch: no
 * padded copy of the image), and a pixel fragment is four consecutive floats of a patch row.  Every output is the same
 * k-ordered fp32 fma chain as the row-packed gather-GEMM plan (sntc_conv_desc.reserved[2] == 1 on a zero-padded image):
 * bit-identical to it, for any batch size and any number of workgroups.
 *   w [k, k, 3, cout]: the Keras HWIO kernel (device pointer); bias [cout] or NULL; act: SNTC_ACT_NONE / RELU / LEAKY_RELU.
 * kind SNTC_SIGNAL_DOWN: the same kernel for tfc.SignalConv2D(corr=True, strides_down=2, padding="same_zeros") on the image -- the
 * first layer of MBT2018Analysis (reference common/transforms.py:152-155; BASELINE configs[1]) -- whose only difference is the
 * padding origin (the kernel is centred: k / 2 in front on both axes); it replaces the generic dword-gather plan
 * there (same products, the row-packed order of summation; tolerance-tested against the oracle, batch-invariant).
 * sntc_rgbconv_supported: 1 where the kernel exists (kind SNTC_CONV2D or SNTC_SIGNAL_DOWN, cin = 3, stride 2, k <= 5, cout in
 * {128, 192, 256}), else 0 -- callers then run the row-packed / generic plan.  x and y < 2 GiB per call. */
typedef struct sntc_rgbconv_plan sntc_rgbconv_plan;
int sntc_rgbconv_supported(int kind, int k, int stride, int cin, int cout, int act);
int sntc_rgbconv_plan_create(int kind, int k, int stride, int cin, int cout, const float* w, const float* bias, int act,
                             void* stream, sntc_rgbconv_plan** plan);
int sntc_rgbconv_plan_update(sntc_rgbconv_plan* plan, const float* w, const float* bias, void* stream);
void sntc_rgbconv_plan_destroy(sntc_rgbconv_plan* plan);
/* Algorithmic 2*MAC FLOPs of one call: 2 n ceil(h/2) ceil(w/2) k k 3 cout (sntc_conv_flops of the layer). */
int64_t sntc_rgbconv_flops(const sntc_rgbconv_plan* plan, int n, int h, int w);
int sntc_rgbconv_forward(const sntc_rgbconv_plan* plan, const float* x, int n, int h, int w, float* y, void* stream);
/* Cap the persistent workgroups of THIS plan's launches (0 = one per CU): tests assert that results do not depend on it. */
int sntc_rgbconv_plan_set_workgroups(sntc_rgbconv_plan* plan, int max_workgroups);
/* ------------------------------------------------------------------------------------------
 * The LAST layer of the multi-layer syntheses -- a 5 x 5 / 2 or 9 x 9 / 4 transposed convolution down to the 3 image channels (reference
 * common/transforms.py:172-175, MBT2018Synthesis: tfc.SignalConv2D(3, (5, 5), corr=False, strides_up=2, padding="same_zeros");
 * :195-206, CNNSynthesis: conv_t_k5s2 = tf.keras.layers.Conv2DTranspose(3, 5, strides=2, padding="SAME"), :85-87) -- as ONE launch of a
 * vector-ALU kernel:
 *   y[n, s h, s w, 3] = conv_transpose(x[n, h, w, cin], w) + bias,   NHWC fp32, no activation (the reference has none there);
 * also :131-134, BLS2017Synthesis: tfc.SignalConv2D(3, (9, 9), corr=False, strides_up=4) (k = 9, stride 4).
 * With three output channels the layer's four output phases are four groups of 3 columns in 32-wide MFMA tiles on the gather
 * GEMM (9.9 TFLOP/s at 8 x 128 x 128 x 192: a quarter of the mbt2018 config's decode); here a block owns 16 x 16 macro pixels, the
 * input channels pass through LDS in 16-channel slabs, a thread runs the 25 taps x 3 outputs of its 2 x 2 output quad with the
 * weights as scalar operands.  fp32 fma chains in another order than sntc_conv_forward's (tolerance-tested against the oracle);
 * an image's results do not depend on the batch.
 *   kind SNTC_CONV2D_TRANSPOSE: w [k, k, 3, cin] (Keras);  SNTC_SIGNAL_UP: w [k, k, cin, 3] (tfc);  bias [3] or NULL.
 * sntc_upsmall_supported: 1 where the kernel exists (those kinds, (k, stride) = (5, 2) or (9, 4), cin % 16 == 0, cout = 3), else 0 -- callers then
 * run sntc_conv_forward. */
typedef struct sntc_upsmall_plan sntc_upsmall_plan;
int sntc_upsmall_supported(int kind, int k, int stride, int cin, int cout);
int sntc_upsmall_plan_create(int kind, int k, int stride, int cin, int cout, const float* w, const float* bias, void* stream,
                             sntc_upsmall_plan** plan);
int sntc_upsmall_plan_update(sntc_upsmall_plan* plan, const float* w, const float* bias, void* stream);
void sntc_upsmall_plan_destroy(sntc_upsmall_plan* plan);
/* Algorithmic 2*MAC FLOPs of one call: 2 n h w k k cin cout (sntc_conv_flops of the layer). */
int64_t sntc_upsmall_flops(const sntc_upsmall_plan* plan, int n, int h, int w);
int sntc_upsmall_forward(const sntc_upsmall_plan* plan, const float* x, int n, int h, int w, float* y, void* stream);
/* ------------------------------------------------------------------------------------------
 * The first layer of the two-layer syntheses (reference common/transforms.py:298-317 TwoLayerSynthesis, :320-361
 * TwoLayerResSynthesis) in ONE launch:  hidden = act(base_conv(y_hat)) [+ res(y_hat)]  -- the tensor the reference hands to
 * its output convolution (:315, :359).  base_conv / res = Conv2DTranspose k x k / stride, SAME (:307-313, :331-338, :351-357);
 * act_kind as in sntc_two_layer_tail (0 none, 1 IGDN1, 2 GDN1, 3 relu, 4 leaky relu) is base_conv's `activation`.
 *   w1 [k, k, (1 + has_res) ch, cin]: the Keras transposed kernel(s), the residual branch's concatenated behind the base
 *   convolution's along the output-channel axis; b1 [(1 + has_res) ch] or NULL; beta [ch], gamma [ch, ch] for act_kind 1 / 2.
 * Indexed by the output-aligned macro pixel a tap is one of nine whole-pixel shifts of the input: a workgroup walks
 * (tile of 256 latent pixels) x (unit of 96 output columns) items -- weights through an LDS-DMA ring, the 16-channel
 * patch slab staged once per slab, every shift a shifted fragment read of it -- dealt dynamically over one workgroup per CU;
 * the activation and the residual add are applied to the accumulators.  Every output is the same k-ordered fp32 fma chain
 * (and the same activation arithmetic) as sntc_conv_forward + stage 1 of sntc_two_layer_tail: bit-identical to them, for any
 * batching.  sntc_syn_supported: 1 where the kernel exists (13 x 13 / 8, 5 x 5 / 2, 3 x 3 / 1 ...: taps within one pixel of
 * the output-aligned source; (1 + has_res) ch in {12, 24, 48}; cin % 16 == 0), else 0 -- callers then run the layers.
 * One call takes up to four batches of DIFFERENT image sizes (sntc_syn_batch: y_hat [n, h, w, cin] -> hidden
 * [n, stride h, stride w, ch]; w <= 127; one image's tensors < 2 GiB): they share the launch's work queue.
 * workspace >= sntc_syn_workspace_bytes(), private to the call until it has run. */
typedef struct sntc_syn_plan sntc_syn_plan;
typedef struct sntc_syn_batch {
  const float* y_hat;
  float* hidden;
  int32_t n, h, w;
  int32_t reserved;
} sntc_syn_batch;
int sntc_syn_supported(int k, int stride, int cin, int ch, int has_res);
int sntc_syn_plan_create(int k, int stride, int cin, int ch, int has_res, int act_kind, const float* w1, const float* b1,
                         const float* beta, const float* gamma, void* stream, sntc_syn_plan** plan);
int sntc_syn_plan_update(sntc_syn_plan* plan, const float* w1, const float* b1, const float* beta, const float* gamma, void* stream);
void sntc_syn_plan_destroy(sntc_syn_plan* plan);
/* Algorithmic 2*MAC FLOPs of `latent_pixels` input pixels (all batches of a call): 2 k^2 cin (1 + has_res) ch each. */
int64_t sntc_syn_flops(const sntc_syn_plan* plan, int64_t latent_pixels);
int64_t sntc_syn_workspace_bytes(const sntc_syn_plan* plan);
int sntc_syn_forward(const sntc_syn_plan* plan, const sntc_syn_batch* batches, int nbatches, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Cap the persistent workgroups of THIS plan's launches (0 = one per CU): tests assert that results do not depend on it. */
int sntc_syn_plan_set_workgroups(sntc_syn_plan* plan, int max_workgroups);
/* The plan's units (tests, tools): up to `capacity` records of four ints (shifts per channel slab; phases held | 32-row tile
 * steps per slab << 8 | mask of the steps that leave the third tile out << 16; the shift list packed four bits per step:
 * low word, high word); returns the number of units. */
int sntc_syn_plan_units(const sntc_syn_plan* plan, int* out, int capacity);
/* The units a layer would get, without a device or a plan (same records as sntc_syn_plan_units; -1 where unsupported). */
int sntc_syn_describe(int k, int stride, int cin, int ch, int has_res, int* out, int capacity);
/* Host-only check of the decomposition (no device): units + packed weights driven through the kernel's loop nest on the CPU
 * against the scatter form of Conv2DTranspose(SAME) on a random h x w input; *max_err = largest absolute difference. */
int sntc_syn_selfcheck(int k, int stride, int cin, int ch, int has_res, int h, int w, unsigned seed, double* max_err);
/* Force the gather-GEMM tile variant of THIS plan (0 = back to the heuristic): profiling and the
 * every-variant parity test only; tile choice never changes results beyond fp32 summation order. */
int sntc_conv_plan_set_tile(sntc_conv_plan* plan, int variant);
/* Schedule switches of THIS plan (tests / profiling).  flags bit 0: 1 (default) lets large launches run on the persistent
 * stream-K workers, 0 forces the static schedule (one workgroup per tile); bit 2 set: bit 1 selects the stage path --
 * 1 direct-to-LDS (buffer_load ... lds), 0 register staging; bit 2 clear: the library default; bit 3: stream-K also for launches of
 * short tiles (< 64 K stages on average), which by default run one workgroup per tile because that is faster; bit 5 set: bit 6
 * selects the stream-K unit order -- 1 column tile outermost (where that twin of the kernel exists), 0 row strip outermost; bit 5
 * clear: column-major where one group's packed weights exceed an XCD's L2.  Every combination
 * produces bit-identical outputs (each element is the same k-ordered fma chain); the switches exist so that a test can
 * assert exactly that. */
int sntc_conv_plan_set_schedule(sntc_conv_plan* plan, int flags);
/* ------------------------------------------------------------------------------------------
 * Split-precision operands (bf16 x 3).  Format S3 of an NHWC tensor with C % 16 == 0: per pixel and 16-channel slab
 * 96 bytes [hi x 16 | mid x 16 | lo x 16] bfloat16 with x = hi + mid + lo (hi = bf16(x), mid = bf16(x - hi),
 * lo = bf16(x - hi - mid)): 6 bytes per element, what a conv plan with reserved[1] == 2 reads.  The reference has no
 * counterpart (fp32 tf.nn.conv2d, common/transforms.py:81-90); these feed the same contractions.
 * ------------------------------------------------------------------------------------------ */
/* out (S3, npix * c * 6 bytes) = split(x [npix, c] fp32) */
int sntc_split3(const float* x, int64_t npix, int c, void* out, void* stream);
/* decoder side of sntc_entropy_scale_normal fused with the split: y_hat = symbols + mu (mu = first half of hyper
 * [npix, 2c], mshyper/models.py:278-279) -> out (S3); y_hat (fp32 [npix, c]) is also written when not NULL */
int sntc_dequant_split3(const int32_t* symbols, const float* hyper, int64_t npix, int c, void* out, float* y_hat,
                        void* stream);
/* Stream-K health.  The persistent stream-K schedule needs every worker of a launch resident at once, which HIP does not
 * promise on a device that other streams or processes share.  A worker that waits in vain (bounded spin) for its neighbour's
 * hand-off no longer traps: it sets bit 0 of a sticky per-device status word and the launch completes with INVALID results.
 * sntc_conv_status exchanges that word with 0 in one atomic on `stream`, copies the old value to *flags and synchronises
 * `stream` -- call it where the host synchronises anyway (the Python driver does: at every device -> host copy of metrics, in
 * compress / decompress, and in encode / decode unless the caller defers the check); launches still in flight on OTHER streams
 * are not covered: join side streams first.  Non-zero means: discard the results since the last check, and re-run after
 * sntc_conv_set_stream_k(0), which makes every later call use the static one-workgroup-per-tile / split-K schedules
 * (bit-identical results).  sntc_conv_status_inject ORs `flags` into the word on `stream` (tests: the raise
 * paths of the callers).  The reference has no counterpart (single stream, cuDNN; common/transforms.py:81-90). */
int sntc_conv_status(int* flags, void* stream);
int sntc_conv_status_inject(int flags, void* stream);
int sntc_conv_set_stream_k(int enabled);
/* The switch's current value (1 = stream-K where the schedule picks it): callers that turn it off around launches which run beside
 * long-lived kernels (Python: ops.static_schedules) put back what they found. */
int sntc_conv_get_stream_k(void);
/* Gather-GEMM tile variant (1..7: 128 x 32v, 8: 64 x 64, 9: 128 x 128 as 64 x 64 per wave, 10: 256 x 128) picked for this call shape,
 * and the number of workgroups it launches; for profiling / roofline bookkeeping. */
int sntc_conv_launch_info(const sntc_conv_plan* plan, int n, int h, int w, int* variant, int* nblocks);
/* 1 if that launch walks its stream-K units column tile outermost (the weights of a few column tiles stay in an XCD's L2 while
 * the row strips stream past: single-group layers whose packed weights exceed 4 MB), 0 for the row-strip-major order.  Profiling
 * only: the kernel's name differs, the bits do not. */
int sntc_conv_launch_order(const sntc_conv_plan* plan, int n, int h, int w, int* column_major);
/* Measured schedule.  Every (tile variant, stream-K / one-workgroup-per-tile) candidate of a plan computes the same k-ordered
 * chains, so the choice is a question of speed only; sntc_conv_plan_tune times them on the caller's buffers for one (n, h, w)
 * (`reps` launches each, HIP events on `stream`, synchronises it) and records the winner in the plan: later calls of that shape
 * run it instead of the cost model's pick (a forced tile / schedule still wins).  `workspace` >= sntc_conv_tune_workspace_bytes().
 * y holds the layer's output afterwards.  A recorded choice can change what sntc_conv_workspace_bytes() reports for that shape: tune
 * (or set a choice) before other threads size their workspaces for it, not while they are between the query and the launch.
 * The reference has no counterpart of its own: TensorFlow's convolutions pick their
 * algorithm by cuDNN autotune the same way (tf.nn.conv2d behind common/transforms.py:81-90). */
int64_t sntc_conv_tune_workspace_bytes(const sntc_conv_plan* plan, int n, int h, int w);
int sntc_conv_plan_tune(sntc_conv_plan* plan, const float* x, int n, int h, int w, float* y, const float* res,
                        const float* aux, void* workspace, size_t workspace_bytes, int reps, int* variant, int* stream_k,
                        void* stream);
/* The candidates sntc_conv_plan_tune would time for this call shape (returns how many were written, < 0 on a bad shape), and a
 * way to record a choice made elsewhere -- e.g. by timing a whole step with several streams in flight, where a schedule
 * measured with the device to itself is not the best one (bench.py does this for its two-stream decode).  Same remark as above:
 * cuDNN's algorithm selection behind tf.nn.conv2d (common/transforms.py:81-90) is the reference-side counterpart. */
int sntc_conv_plan_candidates(const sntc_conv_plan* plan, int n, int h, int w, int* variants, int* stream_k, int capacity);
int sntc_conv_plan_set_choice(sntc_conv_plan* plan, int n, int h, int w, int variant, int stream_k);
int sntc_conv_plan_clear_tuning(sntc_conv_plan* plan);
/* Forget the recorded choice of ONE call shape -- of the whole layer (ncols = 0) or of a column-limited launch (below) -- and keep
 * every other one. */
int sntc_conv_plan_drop_choice(sntc_conv_plan* plan, int n, int h, int w, int ncols);

/* Column-limited launch: the layer restricted to its FIRST `ncols` output channels, y[n, ho, wo, ncols] compact.  A caller that
 * needs only a leading slice of a layer's channels skips the rest of the contraction: the decoder reads mu = the first half of
 * the hyper-synthesis' last layer and never its raw sigma (mshyper/models.py:278-279 splits the two; only the rate needs sigma).
 * A single-group plan packs one weight row per output channel, in channel order, so the launch runs on the SAME plan and the same
 * packed weights with fewer column tiles -- no second plan, no repacking -- and every output it computes is the same k-ordered
 * fp32 fma chain (same split-K factor, same stream-K continuation) as in the whole layer: bit-identical to
 * sntc_conv_forward's y[..., :ncols].
 * Supported (sntc_conv_columns_supported -> 1): plans with one column group whose columns are the output channels (forward
 * convolutions, stride-1 transposed ones), plain fp32 (not bf16 x 3, not row-packed), SNTC_EPI_STORE, 0 < ncols <= cout,
 * ncols % 4 == 0; everything else returns SNTC_ERR_UNSUPPORTED before anything is launched.
 * The queries and the measured-schedule calls below are their sntc_conv_* namesakes for such a launch: tiles, stream-K work
 * units, workspace and candidates are all derived from `ncols`, and a choice recorded for one column count is never applied
 * to another (nor to the whole layer).  Size the workspace with sntc_conv_columns_workspace_bytes for the same `ncols`. */
int sntc_conv_columns_supported(const sntc_conv_plan* plan, int ncols);
int sntc_conv_forward_columns(const sntc_conv_plan* plan, const float* x, int n, int h, int w, float* y, const float* res,
                              const float* aux, void* workspace, size_t workspace_bytes, void* stream, int ncols);
/* The column-limited launch with the decoder's dequantisation in its epilogue: y_hat = v + (float)symbols, where v is what
 * sntc_conv_forward_columns stores and `symbols` is int32 [n, ho, wo, ncols], indexed as the output -- the bits of
 * sntc_dequant_mean(symbols, sntc_conv_forward_columns(...)) without the mu round trip and the second launch.  The plan stays a
 * SNTC_EPI_STORE plan (the encoder's launches of the same plan store plainly); the schedule -- measured or from the cost model --
 * and the workspace are those of the plain column launch at the same (n, h, w, ncols).  Refuses what sntc_conv_forward_columns
 * refuses, and a `symbols` pointer that is null or not 16-byte aligned (SNTC_ERR_UNSUPPORTED, nothing launched). */
int sntc_conv_forward_columns_dequant(const sntc_conv_plan* plan, const float* x, int n, int h, int w, int ncols,
                                      const int32_t* symbols, float* y_hat, void* workspace, size_t workspace_bytes, void* stream);
int64_t sntc_conv_columns_flops(const sntc_conv_plan* plan, int n, int h, int w, int ncols);
int64_t sntc_conv_columns_workspace_bytes(const sntc_conv_plan* plan, int n, int h, int w, int ncols);
/* variant / nblocks as sntc_conv_launch_info, column_major as sntc_conv_launch_order; any of the three may be NULL */
int sntc_conv_columns_launch_info(const sntc_conv_plan* plan, int n, int h, int w, int ncols, int* variant, int* nblocks,
                                  int* column_major);
int64_t sntc_conv_columns_tune_workspace_bytes(const sntc_conv_plan* plan, int n, int h, int w, int ncols);
int sntc_conv_columns_tune(sntc_conv_plan* plan, const float* x, int n, int h, int w, int ncols, float* y, void* workspace,
                           size_t workspace_bytes, int reps, int* variant, int* stream_k, void* stream);
int sntc_conv_columns_candidates(const sntc_conv_plan* plan, int n, int h, int w, int ncols, int* variants, int* stream_k,
                                 int capacity);
int sntc_conv_columns_set_choice(sntc_conv_plan* plan, int n, int h, int w, int ncols, int variant, int stream_k);

/* ------------------------------------------------------------------------------------------
 * Small-channel GDN1 / IGDN1 (C <= 64): wave-shuffle contraction, no MFMA.
 *   replaces GDN1.call, common/transforms.py:26-63.  gamma is [C(in), C(out)], effective values.
 *   alpha in {1,2}; epsilon_is_half selects ^0.5.
 * ------------------------------------------------------------------------------------------ */
int sntc_gdn_small(const float* x, int64_t npix, int c, const float* beta, const float* gamma,
                   int inverse, int alpha, int epsilon_is_half, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Two-layer synthesis tail: h = act(t[..., :Ch]) (+ t[..., Ch:2Ch] if has_res);
 *   x_hat = Conv2DTranspose_{k2 x k2 / s2, SAME}(h) + bias2        (float, NHWC [n, s2*hh, s2*wh, 3])
 *   replaces the IGDN1 + add + out_conv of TwoLayer[Res]Synthesis.call,
 *   common/transforms.py:315-317,359-361 (out_conv kernel [k2,k2,3,Ch]).
 *   act_kind: 0 none, 1 IGDN1, 2 GDN1, 3 relu, 4 leaky_relu.   Ch <= 48, k2 <= 5, s2 == 2.
 * ------------------------------------------------------------------------------------------ */
int sntc_two_layer_tail(const float* t, int n, int hh, int wh, int ch, int has_res, int act_kind,
                        const float* beta, const float* gamma, const float* w2, const float* b2,
                        int k2, int s2, int cout, float* x_hat, void* stream);
/* The same tail with the decoder's last steps fused into the launch: crop to h x w (unpad_images, common/image_utils.py:69-71),
 * floats_to_pixels + quantize_image (common/data_lib.py:48-52, image_utils.py:22-23: (v + .5) * 255, round half to even,
 * saturate) -> pixels uint8 [n, h, w, 3]; with ref (float [n, h, w, 3], normalised) also sse[n] = integer squared error
 * of the two quantised images (mse_psnr, image_utils.py:26-38).  No float reconstruction is written. */
int sntc_two_layer_tail_pixels(const float* t, int n, int hh, int wh, int ch, int has_res, int act_kind,
                               const float* beta, const float* gamma, const float* w2, const float* b2, int k2, int s2,
                               int cout, int h, int w, const float* ref, uint8_t* pixels, uint64_t* sse, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pixel domain
 *   pad_images / unpad_images       common/image_utils.py:41-71
 *   floats_to_pixels + mse_psnr     common/data_lib.py:48-52, common/image_utils.py:22-38
 * ------------------------------------------------------------------------------------------ */
/* Reflect-pad bottom/right: y[n,hp,wp,c] from x[n,h,w,c]  (hp>=h, wp>=w, pads < size). */
int sntc_pad_reflect(const float* x, int n, int h, int w, int c, int hp, int wp, float* y, void* stream);
/* y[n, hp, wp, c] <- x[n, h, w, c] placed at (top, left), zeros elsewhere: the explicit form of Keras SAME padding for a
 * row-packed plan (sntc_conv_desc.reserved[2]).  hp >= top + h, wp >= left + w. */
int sntc_pad_zero(const float* x, int n, int h, int w, int c, int top, int left, int hp, int wp, float* y, void* stream);
/* Crop top-left: y[n,h,w,c] from x[n,hp,wp,c]. */
int sntc_crop(const float* x, int n, int hp, int wp, int c, int h, int w, float* y, void* stream);
/* tf.nn.depth_to_space(x, block), NHWC: y[n, h*block, w*block, c/block^2] with input channel (dy*block + dx)*(c/block^2) + k
 * going to output pixel (iy*block + dy, ix*block + dx), channel k -- the upsampling steps of
 * TwoLayerResSynthesis(res_type="d2s"), common/transforms.py:341-348. */
int sntc_depth_to_space(const float* x, int n, int h, int w, int c, int block, float* y, void* stream);
/* y[npix, ca + cb] = [a | b] along the channel axis (tf.concat(..., axis=-1)); b == NULL appends a channel of ones and cb - 1 zero
 * channels instead: the constant input of JPEGLikeSynthesis(use_offset=True), common/transforms.py:291-293, padded to a 16-channel slab. */
int sntc_concat_channels(const float* a, int ca, const float* b, int cb, int64_t npix, float* y, void* stream);
/* Quantise both images to uint8 the reference's way ((v+.5)*255, round-half-even, saturate) and
 * accumulate the per-image integer sum of squared differences.  x_hat may be strided (crop fused):
 * element (b,i,j,k) at x_hat[((b*hs + i)*ws + j)*c + k].  pixels_out (uint8 [n,h,w,c]) may be NULL.
 * sse_out: uint64 [n], OVERWRITTEN (zeroed on stream first).  x == NULL: only quantise x_hat into
 * pixels_out (the decoder's last step); sse_out is then ignored. */
int sntc_pixels_sse(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws,
                    uint8_t* pixels_out, unsigned long long* sse_out, void* stream);
/* The integer squared error of decoded uint8 pixels [n,h,w,c] against x [n,h,w,c] quantised the same way (the rule of
 * sntc_pixels_sse; common/data_lib.py:48-52, common/image_utils.py:22-23) over every block x block pixel block: out uint32
 * [n][ceil(h / block)][ceil(w / block)], OVERWRITTEN; blocks at the right and bottom edges may be ragged.  Integers end to end
 * (one wave per block, one store per block): exact, and the per-image sums are sntc_pixels_sse's.  block^2 c 255^2 must stay
 * below 2^32 (SNTC_ERR_BAD_SHAPE otherwise). */
int sntc_block_sse(const float* x, const uint8_t* pixels, int n, int h, int w, int c, int block, uint32_t* out, void* stream);
/* Training-mode distortion (SGA): sum over (255*(x - x_hat))^2 in float, per image, double out. */
int sntc_float_sse(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws,
                   double* sse_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Entropy models (compression=False paths: rate *estimates*, as the reference evaluates them)
 * ------------------------------------------------------------------------------------------ */
/* tfc.DeepFactorized parameters for C channels, `nlayers` = len(num_filters)+1 affine layers of
 * widths 1 -> f1 -> ... -> 1 (widths[nlayers+1], each <= 4).  Raw TFC variables (softplus / tanh
 * are applied inside): matrices[k] [C,f_{k+1},f_k], biases[k] [C,f_{k+1}], factors[k] [C,f_{k+1}],
 * concatenated per kind in layer order as host float arrays. */
typedef struct sntc_prior sntc_prior;
int sntc_prior_create(int channels, int nlayers, const int* widths, const float* matrices,
                      const float* biases, const float* factors, void* stream, sntc_prior** prior);
void sntc_prior_destroy(sntc_prior* prior);

/* tfc.ContinuousBatchedEntropyModel(NoisyDeepFactorized, coding_rank=3, compression=False)
 *   __call__(z, training=False): mshyper/models.py:249-255, factorized/models.py:101-105.
 * z[n, hw, C] -> z_hat = round(z) (float) and bits[n] (double, -sum log2 p).
 * values_only != 0: skip rounding and evaluate bits at z as given (log_prob of an explicit sample,
 *   mshyper/models.py:262-268). */
int sntc_entropy_factorized(const sntc_prior* prior, const float* z, int n, int64_t hw, float* z_hat,
                            double* bits, int values_only, void* stream);

/* tfc.LocationScaleIndexedEntropyModel(NoisyNormal, 64, SCALE_FN, coding_rank=3,
 *   compression=False)(y, indexes=exp(raw), loc=mu, training=False): mshyper/models.py:273-279.
 * hyper[n, hw, 2C] holds mu = hyper[..., :C] and raw = hyper[..., C:]  (tf.split + tf.exp fused).
 * Outputs: y_hat = round(y - mu) + mu (float), symbols = round(y - mu) as int32 (may be NULL),
 * bits[n] (double).  values_only != 0: y is an explicit sample; bits evaluated at y - mu without
 * rounding, y_hat/symbols untouched (mshyper/models.py:285-291). */
int sntc_entropy_scale_normal(const float* y, const float* hyper, int n, int64_t hw, int c,
                              float* y_hat, int32_t* symbols, double* bits, int values_only,
                              void* stream);
/* Decoder-side dequantisation: y_hat = symbols + mu  (mu = hyper[..., :C]). */
int sntc_dequant_scale_normal(const int32_t* symbols, const float* hyper, int n, int64_t hw, int c,
                              float* y_hat, void* stream);
/* The same from a mu tensor with `mu_stride` floats per pixel (>= c, a multiple of 4): c for the compact output of a mean-only
 * hyper-synthesis (sntc_conv_forward_columns), 2 c for the full [mu | raw] rows. */
int sntc_dequant_mean(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride, float* y_hat,
                      void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Bitstream: table-driven 64-way interleaved rANS, 16-bit quantised CDFs.  The reference has no
 *   bitstream (compression=False at mshyper/models.py:246-251; its bpp is the estimate); these entry points make
 *   `decode` a real codec.  One stream per (image, segment); an image's elements_per_image values (flat, in memory
 *   order) are cut into `segments` runs of sntc_rans_cap_words()/2 - 64 elements (a multiple of 64).
 *   Tables: cdf = uint16, concatenated, table t holds cdf[0..n) (cdf[n] = 65536 implicit; pad the array to an even
 *   count); meta = uint32 [ntables][2] = { offset into cdf, (n << 16) | (vmin & 0xffff) }; the last symbol of every
 *   table is ESCAPE, followed in the stream by value + 32768 as a raw 16-bit word.
 *   Stream = [lanes x (state hi, state lo)] [16-bit words in decode order]  (format: csrc/rans.hip header);
 *   lanes in {8, 16, 32, 64}: element lanes*j + l belongs to lane l at step j; fewer lanes = fewer flushed bytes.
 * ------------------------------------------------------------------------------------------------------- */
int64_t sntc_rans_cap_words(int64_t elems_per_image, int segments);
/* scratch: uint16 [nimages * segments][cap_words]; stream s ends up in the LAST len_words[s] words of its row. */
int sntc_rans_encode(const int32_t* values, const uint16_t* table_ids, int nimages, int64_t elems_per_image, int segments,
                     int lanes, const uint16_t* cdf, const uint32_t* meta, int ntables, int total_entries, int64_t cap_words,
                     uint16_t* scratch, int32_t* len_words, void* stream);
/* gathers the streams into one payload; offsets int64 [nstreams + 1] = exclusive prefix sum of len_words */
int sntc_rans_compact(const uint16_t* scratch, int64_t cap_words, const int32_t* len_words, const int64_t* offsets,
                      int nstreams, uint16_t* payload, void* stream);
/* bad_streams (int32[1], device) counts streams that did not end at their initial state / length: corruption.
 * dec / lut / lut_meta (all three or none; NULL = the plain decoder, a binary search of cdf per symbol) are the decoder's own
 *   view of the same tables, which it keeps in LDS:
 *   dec      uint32, table t's entry s at dec[offset_t + 3 t + s] = (cdf[s] << 16) | (freq[s] - 1), three 0xffffffff after every
 *            table, the array padded to a multiple of 4 entries (total_entries + 3 ntables, rounded up);
 *   lut      per table a START TABLE of 2^bits uint16 entries, lut[lut_off + b] = the largest symbol s with
 *            cdf[s] <= b << (16 - bits), 0 <= bits <= 16; lut_meta[t] = (lut_off << 5) | bits; lut_entries a multiple of 8 and
 *            <= sntc_rans_lut_budget(ntables, total_entries), the room the other tables leave in a CU's LDS.
 *   The decoded values do not depend on them; with about one start entry per symbol a step costs three LDS round trips
 *   instead of log2(n) + 2. */
int64_t sntc_rans_lut_budget(int ntables, int total_entries);
int sntc_rans_decode(const uint16_t* payload, const int64_t* offsets, const uint16_t* table_ids, int nimages,
                     int64_t elems_per_image, int segments, int lanes, const uint16_t* cdf, const uint32_t* meta, int ntables,
                     int total_entries, const uint32_t* dec, const uint16_t* lut, const uint32_t* lut_meta, int lut_entries,
                     int32_t* values, int32_t* bad_streams, void* stream);
/* The same coder for ONE latent whose table is its channel (the factorized-prior model, reference factorized/models.py:101-124:
 *   one deep-factorized density per channel), straight from / to the float latents: no table-id tensor, no int32 copy.
 *   y / y_hat float [nimages][elems_per_image], flat NHWC; the table of element e of an image is e % channels, the table set has
 *   `channels` tables, elems_per_image % channels == 0 (checked).  The encoder codes symbol = (int)rintf(y[e]) (round half to
 *   even, as sntc_round_to_int) and, where y_hat is not NULL, writes (float)symbol there; the decoder writes (float)value.
 *   Streams, scratch, len_words, offsets, cap_words, segments, lanes, bad_streams: as above, and the words of a stream are those
 *   sntc_rans_encode emits for the same integers with sntc_channel_table_ids -- either decoder reads either encoder's streams.
 *   dec / lut / lut_meta: as sntc_rans_decode (all three or none); these kernels keep no id ring in LDS, so every lut_entries
 *   within sntc_rans_lut_budget() fits, and a little more.  Tables too wide for a CU's LDS are read from global memory.
 *   A value outside [-32768, 32767] is coded clamped (an escaped value travels in 16 bits); y_hat of the encoder is not. */
int sntc_rans_encode_channels(const float* y, int nimages, int64_t elems_per_image, int channels, int segments, int lanes,
                              const uint16_t* cdf, const uint32_t* meta, int total_entries, int64_t cap_words, uint16_t* scratch,
                              int32_t* len_words, float* y_hat, void* stream);
int sntc_rans_decode_channels(const uint16_t* payload, const int64_t* offsets, int nimages, int64_t elems_per_image, int channels,
                              int segments, int lanes, const uint16_t* cdf, const uint32_t* meta, int total_entries,
                              const uint32_t* dec, const uint16_t* lut, const uint32_t* lut_meta, int lut_entries, float* y_hat,
                              int32_t* bad_streams, void* stream);
/* What the streams of sntc_rans_encode pay for the symbols of `values`, without coding them (the reference has no bitstream,
 *   compression=False at mshyper/models.py:246-251, and scores latents by the continuous estimate only):
 *   cost[b] = sum over image b's elements of cost_q[offset_t + symbol], t = the element's table id and symbol = value - vmin_t,
 *   or ESCAPE (the table's last symbol) when that is < 0 or >= n_t - 1 -- the encoder's own rule.
 *   cost_q: uint32, one entry per cdf entry at the same offsets, = rint((16 - log2(freq)) * 65536), ESCAPE entries + 16 * 65536
 *   (the raw 16-bit value): the unit is 2^-16 bit.  cost: uint64 [nimages], zeroed by the call.  All sums are integers:
 *   the result is the exact sum whatever the launch geometry.  Table ids must be < ntables (not checked, as in the coder).
 *   Not included: the flushed lane states (32 bits per lane and stream) and the states' renormalisation slack. */
int sntc_rans_cost(const int32_t* values, const uint16_t* table_ids, int nimages, int64_t elems_per_image, const uint32_t* meta,
                   int ntables, int total_entries, const uint32_t* cost_q, uint64_t* cost, void* stream);
/* table id of every y element = round(clamp(exp(raw), 0, 63)), raw = hyper[..., c:]; of every z element = channel */
int sntc_scale_table_ids(const float* hyper, int64_t npix, int c, uint16_t* table_ids, void* stream);
/* table id = channel (deep-factorized prior: one table per channel). */
int sntc_channel_table_ids(int64_t npix, int c, uint16_t* table_ids, void* stream);
int sntc_round_to_int(const float* x, int64_t total, int32_t* out, void* stream);
int sntc_int_to_float(const int32_t* x, int64_t total, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Quantisation steps off the scale ladder (csrc/quant_step.hip): the reference quantises y - mu with step 1
 *   and indexes its 64 tables by exp(raw) (mshyper/models.py:273-279); these entry points generalise both lines to a step
 *   r^k, r = exp((ln 256 - ln 0.11) / 63), k an integer ladder index in [-32, 32]:
 *     symbol   = (int)rintf((y - mu) * inv_step)   inv_step = float32(r^-k); a float32 subtract, then a float32 multiply
 *     table id = clamp(base id - k, 0, 63)         base id = sntc_scale_table_ids; the end tables stay off the ladder's ends
 *     y_hat    = fmaf(step, (float)symbol, mu)     step = float32(r^k)
 *   sigma_i / r^k = sigma_(i-k): the symbols of step k are distributed as table i - k describes, so the tables, the coder and
 *   the decoder serve every step.  With step = inv_step = 1.0f, k = 0 these are the symbols of sntc_entropy_scale_normal, the
 *   ids of sntc_scale_table_ids and the values of sntc_dequant_mean, bit for bit.
 *   y / symbols / ids: [n][hw][c], c % 4 == 0; mu: `mu_stride` floats per pixel as in sntc_dequant_mean; n <= 65535.
 * ------------------------------------------------------------------------------------------------------- */
/* One step per image: inv_step float [n], shift (= k) int32 [n], both on the device.  Writes symbols int32 and the shifted
 * table_ids uint16.  y / mu / symbols 16-byte aligned, the id arrays 8-byte aligned (checked). */
int sntc_step_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                      const float* inv_step, const int32_t* shift, int32_t* symbols, uint16_t* table_ids, void* stream);
/* The id rule alone, for a decoder (it has the ids of its hyper-synthesis and no y): table_ids = clamp(base_ids - shift[image], 0, 63),
 * [n][elems_per_image]. */
int sntc_step_table_ids(const uint16_t* base_ids, int n, int64_t elems_per_image, const int32_t* shift, uint16_t* table_ids,
                        void* stream);
/* sntc_dequant_mean at one step per image: step float [n] on the device. */
int sntc_dequant_step(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* step,
                      float* y_hat, void* stream);
/* What sntc_rans_cost would return for the symbols and ids of sntc_step_symbols at each of `nsteps` candidate steps shared by
 *   the batch (1 <= nsteps <= 16; inv_step float [nsteps], shift int32 [nsteps], on the device), in ONE pass over y, mu and the
 *   base ids (10 bytes per element), without writing a symbol: cost uint64 [n][nsteps], zeroed by the call, in units of
 *   2^-16 bit.  meta / cost_q / ntables / total_entries: as sntc_rans_cost; the set holds the ladder's 64 tables first
 *   (ntables >= 64).  All sums are integers: the result is exact whatever the launch geometry.  Pointers that are not aligned
 *   for 16-byte loads (y, mu) / 8-byte loads (base_ids) take an element-wise path with the same result. */
int sntc_step_ladder_cost(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                          const float* inv_step, const int32_t* shift, int nsteps, const uint32_t* meta, int ntables,
                          int total_entries, const uint32_t* cost_q, uint64_t* cost, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The same three rules with the ladder index varying per latent POSITION (csrc/quant_step.hip; region-of-interest coding,
 *   wire format 7): kmap int8 [n][hw], one index k in [-32, 32] per position, shared by its c channels.  step / inv_step come
 *   from ONE table the host uploads, lut float [2][65]: lut[k + 32] = float32(r^k), lut[65 + k + 32] = float32(r^-k) (float64,
 *   rounded once; never recomputed on the device).  The kernels clamp every index they read into [-32, 32]: no byte of a map
 *   can read outside lut.  With a constant map: the per-image entry points above at that index, bit for bit.
 *   Sizes and alignment as above (checked).
 * ------------------------------------------------------------------------------------------------------- */
int sntc_step_map_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                          const int8_t* kmap, const float* lut, int32_t* symbols, uint16_t* table_ids, void* stream);
/* The decoder's half: table_ids = clamp(base_ids - kmap[image][position], 0, 63), [n][hw][c]. */
int sntc_step_map_table_ids(const uint16_t* base_ids, int n, int64_t hw, int c, const int8_t* kmap, uint16_t* table_ids,
                            void* stream);
int sntc_dequant_step_map(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride, const int8_t* kmap,
                          const float* lut, float* y_hat, void* stream);
/* sntc_step_ladder_cost over a map: candidate j (base int32 [nsteps] on the device, 1 <= nsteps <= 16) prices position p at
 *   the index clamp(base[j] + offsets[image][p], -32, 32); offsets int8 [n][hw].  cost uint64 [n][nsteps], zeroed by the call.
 *   One pass over y, mu and the ids; integer sums; the element-wise path for unaligned pointers, as there. */
int sntc_step_map_ladder_cost(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                              const int8_t* offsets, const float* lut, const int32_t* base, int nsteps, const uint32_t* meta,
                              int ntables, int total_entries, const uint32_t* cost_q, uint64_t* cost, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Rate-distortion optimised quantisation (csrc/rdoq.hip, rule in csrc/rdoq_rules.h; DESIGN.md 4.7 "RDOQ").  The reference
 *   rounds y - mu to the nearest integer (mshyper/models.py:273-279) and so do the step kernels above; these two choose, per
 *   element, among the nearest integer and its neighbours towards zero by exact rate + weighted squared error.  With the three
 *   rules above, d = y - mu, u = d * inv_step (float32), s0 = (int)rintf(u), t = clamp(base id - k, 0, 63) and
 *   price(s) = cost_q[offset_t + symbol of s in table t] (sntc_rans_cost's entry, ESCAPE included):
 *     enable[image] == 0 or s0 == 0:  symbol = s0
 *     else the candidates, in order:  s0;  a = s0 - sign(s0);  0, if flags & 1 and a != 0
 *       J(s) = fadd(fmul(weight[channel], fmul(e, e)), (float)price(s)),  e = fsub(u, (float)s)
 *       every operation one float32 rounding, nothing fused; the smallest J wins, a later candidate only on strict <
 *       (a NaN J never displaces s0, a tie keeps the nearer symbol)
 *   table_ids are those sntc_step_symbols / sntc_step_map_symbols write: the symbols go into ordinary wire format 3 / 5 / 7.
 *   With every enable 0 the outputs are those entry points', bit for bit.  s0 is the nearest integer, so with weight >= 0 a
 *   change is always to a strictly cheaper symbol: per image sntc_rans_cost of these symbols <= that of the plain ones, < where
 *   changed > 0.
 *   weight float [c] (cost_q units, 2^-16 bit, per squared symbol-unit error), enable int32 [n], both on the device; meta /
 *   ntables / total_entries / cost_q as sntc_rans_cost, the set holding the ladder's 64 tables first (ntables >= 64); staged in
 *   LDS where they fit, read from memory otherwise, same result.  changed (optional, may be null) int32 [n], zeroed by the call:
 *   the elements of each image written != s0, an exact integer whatever the launch geometry.  y / mu / symbols / weight
 *   16-byte aligned, the id arrays 8-byte aligned, c % 4 == 0, mu_stride >= c and % 4 == 0, 1 <= n <= 65535 (checked,
 *   SNTC_ERR_BAD_SHAPE before any launch).
 * ------------------------------------------------------------------------------------------------------- */
int sntc_rdoq_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                      const float* inv_step, const int32_t* shift, const float* weight, const int32_t* enable, int flags,
                      const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, int32_t* symbols,
                      uint16_t* table_ids, int32_t* changed, void* stream);
/* The same with k and inv_step per latent position: kmap int8 [n][hw], lut float [2][65] as in sntc_step_map_symbols. */
int sntc_rdoq_map_symbols(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const uint16_t* base_ids,
                          const int8_t* kmap, const float* lut, const float* weight, const int32_t* enable, int flags,
                          const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q, int32_t* symbols,
                          uint16_t* table_ids, int32_t* changed, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Requantisation: the symbols of a coarser step from the symbols a file holds, without y and without pixels
 *   (csrc/quant_step.hip, DESIGN.md 4.7 "transcode").  The reference quantises once, from y, with step 1
 *   (mshyper/models.py:273-279) and has no second rate; here the source is what its decoder would hand the synthesis.  Per
 *   element, at the source index k0 = src_map[image][position] and a destination index k1, with the three rules above and
 *   nothing else:
 *     y_hat0 = fmaf(lut[k0 + 32], (float)s0, mu)                        sntc_dequant_step_map's value, rounded to float32 once
 *     s1     = (int)rintf((y_hat0 - mu) * lut[65 + k1 + 32])            sntc_step_map_symbols' symbol of it
 *     t1     = clamp(base id - k1, 0, 63)
 *   -- sntc_step_map_symbols / sntc_step_map_ladder_cost on the stored values of sntc_dequant_step_map, bit for bit, without
 *   the y_hat tensor.  src_map / dst_map int8 [n][hw], clamped into [-32, 32] as every map; a unit or per-image grid is a
 *   constant map.  lut float [2][65] as above.  Sizes and alignment as above (checked).
 * ------------------------------------------------------------------------------------------------------- */
/* k1 = dst_map[image][position].  Writes out_symbols int32 and out_table_ids uint16 in one pass.  symbols / mu / out_symbols
 * 16-byte aligned, the id arrays 8-byte aligned (checked). */
int sntc_step_requant_symbols(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                              const uint16_t* base_ids, const int8_t* src_map, const int8_t* dst_map, const float* lut,
                              int32_t* out_symbols, uint16_t* out_table_ids, void* stream);
/* sntc_step_map_ladder_cost of the requantised symbols: candidate j (shift int32 [nsteps] on the device, 1 <= nsteps <= 16)
 *   prices every element at k1 = clamp(clamp(src_map[image][p]) + shift[j], -32, 32).  cost uint64 [n][nsteps], zeroed by the
 *   call, exact integer sums in 2^-16 bit.  One pass over symbols, mu, the ids and the map (about 10 bytes per element); no
 *   y_hat or symbol tensor is written; the element-wise path for unaligned pointers, as there. */
int sntc_step_requant_ladder_cost(const int32_t* symbols, const float* mu, int n, int64_t hw, int c, int mu_stride,
                                  const uint16_t* base_ids, const int8_t* src_map, const float* lut, const int32_t* shift,
                                  int nsteps, const uint32_t* meta, int ntables, int total_entries, const uint32_t* cost_q,
                                  uint64_t* cost, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The distortion side of the ladder (csrc/quant_step.hip, DESIGN.md 4.7 "quality target"): what every candidate step
 *   DECODES to, in one pass.  The reference decodes y_hat = round(y - mu) + mu once per evaluation (mshyper/models.py:273-279);
 *   here, per element and candidate j (1 <= nsteps <= 16), with the three rules above and nothing else,
 *     s = (int)rintf((y - mu) * inv_step[j]),  y_hat[j][image][position][channel] = fmaf(step[j], (float)s, mu)
 *   -- sntc_dequant_step of sntc_step_symbols at that step, bit for bit, without a symbol tensor.  The symbol is NOT clamped:
 *   it is the one coded_cost decodes, not the file's 16-bit escape.  y_hat float [nsteps][n][hw][c]: candidate j is a contiguous
 *   batch of n latents, so the candidates go through the decoder as ONE batch of nsteps n.  y and mu are read once (8 bytes per
 *   element) and feed nsteps stores (4 nsteps bytes): a store stream, no atomics, no LDS.  inv_step / step float [nsteps] on the
 *   device.  mu_stride is c or 2 c; 1 <= n <= 65535; any c >= 1.  16-byte loads and stores where y, mu and y_hat are 16-byte
 *   aligned and c % 4 == 0, an element-wise path with the same result otherwise. */
int sntc_step_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const float* inv_step,
                             const float* step, int nsteps, float* y_hat, void* stream);
/* The same over a map: candidate j (base int32 [nsteps] on the device) quantises position p at the index
 *   clamp(base[j] + offsets[image][p], -32, 32), offsets int8 [n][hw], step and inverse step read from lut float [2][65] as in
 *   sntc_step_map_symbols -- sntc_dequant_step_map of sntc_step_map_symbols on that map, bit for bit. */
int sntc_step_map_ladder_dequant(const float* y, const float* mu, int n, int64_t hw, int c, int mu_stride, const int8_t* offsets,
                                 const float* lut, const int32_t* base, int nsteps, float* y_hat, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The coded pixel residual layer (csrc/residual.hip, rule in csrc/residual_rules.h; wire format 8, DESIGN.md 4.7 "residual
 *   layer").  The reference writes no file and bounds no pixel (mshyper/models.py:246-251, :313-317); this layer codes, over any
 *   decoded base picture, the integers that bring every pixel within max_error = delta of the uint8 original (0: lossless).
 *   Images are [n][h][w][c], 1 <= c <= 4, 1 <= n <= 65535, h w c < 2^31; base uint8 = the decoded base picture; x8 = the
 *   original quantised as sntc_pixels_sse quantises it: (v + .5) 255, round half to even, saturate.  With m = 2 delta + 1, in
 *   integers:
 *     q  = sgn(x8 - base) ((|x8 - base| + delta) div m)                 |q| <= (255 + delta) div m
 *     x~ = clip(base + q m, 0, 255)                                     |x8 - x~| <= delta
 *     class(i, j, k) = level c + k,  level = 0 if a == 0 else min(7, floor(log2 a) + 1),
 *     a = |base(i, min(j+1, w-1), k) - base(i, max(j-1, 0), k)| + |base(min(i+1, h-1), j, k) - base(max(i-1, 0), j, k)|
 *   Refused with SNTC_ERR_BAD_SHAPE before any launch: a null pointer, max_error outside 0 .. 127, c outside 1 .. 4, a
 *   non-positive size.  16-byte loads and stores where the pointers are aligned for them and h w c % 4 == 0, an element-wise
 *   path with the same integers otherwise.  None of them allocates or synchronises.
 * ------------------------------------------------------------------------------------------------------- */
/* q int32 [n][h][w][c] and hist uint32 [n][8 c][511] (OVERWRITTEN): hist[image][class][q + 255] = how many values of that class
 * took q.  The counts are integer atomics: exact whatever the launch geometry. */
int sntc_residual_quantize(const float* x, const uint8_t* base, int n, int h, int w, int c, int max_error, int32_t* q,
                           uint32_t* hist, void* stream);
/* table_ids uint16 [n][h][w][c] = min(choice[image][class], 63), choice uint8 [n][8 c] on the device: the table the encoder
 * chose per (image, class).  The encoder and the decoder call it on the same base picture. */
int sntc_residual_table_ids(const uint8_t* base, const uint8_t* choice, int n, int h, int w, int c, uint16_t* table_ids,
                            void* stream);
/* out uint8 [n][h][w][c] = x~ for any int32 q; out_of_range int32 [1] on the device (zeroed by the call) counts the values with
 * |q| > (255 + delta) div m, which no encoder writes: the decoder's corruption count, read where bad_streams is read. */
int sntc_residual_apply(const uint8_t* base, const int32_t* q, int n, int h, int w, int c, int max_error, uint8_t* out,
                        int32_t* out_of_range, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Tiled files (csrc/tiles.hip, rule in csrc/tile_rules.h; wire format 9, DESIGN.md 4.7 "tiled files").  The reference has no
 *   bitstream at all (mshyper/models.py:246-251: compression=False), so it has no tiles either; these two entry points are the
 *   pixel ends of a file whose picture is cut into independently coded, overlapping tiles.  Per axis, for a length L, a tile
 *   size T and an overlap O (T >= 4, T % 4 == 0, 0 <= O <= min(T / 4, 1024)), in integers:
 *     R = max(1, L div T) tiles; the core of tile r is [r T, (r + 1) T), the last core runs to L (length in [T, 2 T))
 *     extent(r) = the core grown by O on each interior side, clipped to [0, L)
 *     extents r and r + 1 meet exactly in the band [(r + 1) T - O, (r + 1) T + O); bands are disjoint
 *     at band offset j tile r + 1 weighs 2 j + 1, tile r weighs 4 O - (2 j + 1), denominator 4 O; elsewhere weight 1 over 1
 *     a 2-D weight is the product of the axis weights, D = Dy Dx, value = (sum_t w_t v_t + D / 2) div D
 *   Neither allocates or synchronises.
 * ------------------------------------------------------------------------------------------------------- */
/* out float [ntiles][th][tw][c] = x[image][y0 : y0 + th][x0 : x0 + tw][:] for the tiles of one shape class; x float [n][H][W][c].
 * rects int32 [ntiles][3] = (image, y0, x0) ON THE HOST: checked here -- a rect that leaves the image is refused with
 * SNTC_ERR_BAD_SHAPE before any launch -- and handed to the kernel as arguments, 256 tiles per launch.  16-byte copies where
 * the rows of both sides are aligned for them, coalesced dwords otherwise.  th tw c < 2^31. */
int sntc_tiles_extract(const float* x, int n, int H, int W, int c, const int32_t* rects, int ntiles, int th, int tw, float* out,
                       void* stream);
/* out uint8 [n][rh][rw][c] = the window [ry, ry + rh) x [rx, rx + rw) of the picture the tiles make, every value written once
 * from the 1, 2 or 4 tiles that cover its pixel, blended by the integer rule above: no atomics on pixels, no accumulator, the
 * same bytes from any launch.  tile_ptrs: a device array of n R C device pointers, (image, tile row, tile column) order, each to
 * that tile's uint8 [extent height][extent width][c] or NULL for a tile that was not decoded.  A pixel that needs a NULL tile is
 * written as 0 and counted in missing int32 [1] on the device (zeroed by the call); a NULL tile the window does not touch is
 * never read.  out may start at any byte.  1 <= c <= 4, n <= 65535.  Refused with SNTC_ERR_BAD_SHAPE before
 * any launch: a null argument, a tile / overlap outside the rule, a window that leaves the picture. */
int sntc_tiles_assemble(const uint8_t* const* tile_ptrs, int n, int H, int W, int c, int tile, int overlap, int ry, int rx, int rh,
                        int rw, uint8_t* out, int32_t* missing, void* stream);

/* ------------------------------------------------------------------------------------------
 * SSIM / MS-SSIM statistics (eval-only quality metrics, reference mshyper/models.py:321-336 ->
 *   tf.image.ssim / tf.image.ssim_multiscale).  Images are float NHWC holding pixel
 *   values (0..max_val), c in {1, 3}.
 * ------------------------------------------------------------------------------------------ */
/* One scale: 11 x 11 Gaussian (sigma 1.5) VALID moments; ssim_sum[n*c] = sum over filter outputs of
 * luminance*cs, cs_sum[n*c] = sum of cs (both OVERWRITTEN).  Divide by (h-10)(w-10) for the means. */
int sntc_ssim_scale(const float* a, const float* b, int n, int h, int w, int c, float max_val, double* ssim_sum,
                    double* cs_sum, void* stream);
/* 2 x 2 average pooling to ceil(h/2) x ceil(w/2); odd sizes repeat the last row / column (tf.pad SYMMETRIC). */
int sntc_avgpool2_symmetric(const float* x, int n, int h, int w, int c, float* y, void* stream);
/* crop + floats_to_pixels (round-half-even, clamp 0..255) kept as float: the SSIM input. */
int sntc_pixels_float(const float* x_hat, int n, int h, int w, int c, int hs, int ws, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * (MS-)SSIM as a differentiable distortion (csrc/msssim_grad.hip; the quality is reference mshyper/models.py:321-331,
 *   DESIGN.md 4.6): D = 1 - mean_B q_i on the UNROUNDED, unclamped floats a = (x + .5) 255, b = (x_hat cropped + .5) 255,
 *   max_val 255.  q_i: single-scale SSIM when both sides are < 160, five-scale MS-SSIM otherwise; every factor max(., 0);
 *   per channel prod_k f_k^{w_k}, then the mean over channels.  A factor clamped at 0 contributes zero gradient and zeroes the
 *   gradient of its whole (image, channel) product.  None of these entry points allocates or synchronises.
 * ------------------------------------------------------------------------------------------ */
/* a[n,h,w,c], b[n,h,w,c] as above from x[n,h,w,c] and x_hat[n,hs,ws,c]; sse[n] (OVERWRITTEN) as sntc_distortion_grad leaves it
 * (reference mshyper/models.py:321-331 on the training-mode floats of :313-317). */
int sntc_msssim_inputs(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws, float* a, float* b,
                       double* sse, void* stream);
/* Device-side finish of the 5-factor product (reference mshyper/models.py:321-331): sums[scales, 2, n, c] are the outputs of
 * sntc_ssim_scale per scale ([k][0] ssim, [k][1] cs), counts[scales] / weights[scales] HOST arrays (filter outputs per scale;
 * the MS-SSIM power factors, may be NULL when scales == 1 = single-scale SSIM).  -> q[n] (float64) and
 * coef[scales, n, c] = d(weight * q_i) / d(sum_k): the factor of the cs map's gradient on scales 0 .. last-1 and of the ssim
 * map's on the last (or single) scale, 0 for a product with a clamped factor.  weight = -lambda / n for rd_loss. */
int sntc_msssim_finish(const double* sums, const double* counts, const double* weights, int scales, int n, int c, double weight,
                       double* q, float* coef, void* stream);
/* One scale of the gradient (reference mshyper/models.py:321-331), c in {1, 3}, one launch: for every pixel r of b
 *   g(r) = coef[n, c] ((w * A)(r) + a(r) (w * B)(r) + 2 b(r) (w * C)(r)) + 1/4 g_coarse(floor(r / 2)) [x 2 per replicated edge]
 * with A, B, C the partial derivatives of the cs map (use_lum = 0) or the ssim = luminance * cs map (use_lum = 1) w.r.t.
 * mu_b, E[ab], E[a^2 + b^2] at each filter output, and w * the full (adjoint-of-VALID) 11-tap separable correlation.
 * g_coarse[n, ceil(h/2), ceil(w/2), c] is the next scale's gradient or NULL.  g[n, hs, ws, c] (hs >= h, ws >= w) is
 * OVERWRITTEN with out_scale * g(r), zeros in the margin (scale 0: the padded x_hat shape and out_scale = 255). */
int sntc_ssim_scale_grad(const float* a, const float* b, int n, int h, int w, int c, float max_val, const float* coef, int use_lum,
                         const float* g_coarse, int hs, int ws, float out_scale, float* g, void* stream);
/* Adjoint of sntc_avgpool2_symmetric (reference mshyper/models.py:321-331, the pooling between MS-SSIM scales):
 * g_fine[n, h, w, c] (OVERWRITTEN) from g_coarse[n, ceil(h/2), ceil(w/2), c]; the replicated last row / column of an odd size
 * receives both of its contributions. */
int sntc_avgpool2_symmetric_grad(const float* g_coarse, int n, int h, int w, int c, float* g_fine, void* stream);

/* ------------------------------------------------------------------------------------------
 * SGA iterative inference (config 5): element-wise pieces of Model.itinf_train_step,
 *   mshyper/models.py:397-408 with frame_loss_given_latent_rvs(training=True), :260-268,285-291,343.
 *   The contractions of the backward pass are sntc_conv_forward calls: the input gradient of
 *   Conv2DTranspose(k, s, SAME) with kernel W[kh,kw,Cout,Cin] is SNTC_CONV2D with the same array
 *   read as [kh,kw,Cin'=Cout,Cout'=Cin]; relu / leaky-relu masks ride on SNTC_EPI_MASK_*.
 * sga_round (common/latent_rvs_utils.py:8-48): logits = (-atanh(clip(u - floor u))/tau,
 *   -atanh(clip(ceil u - u))/tau), w = softmax((logits + Gumbel)/tau), sample = w0 floor + w1 ceil.
 *   noise: NULL -> counter-based generator keyed by (seed, step, element); else float [.., 2]
 *   Gumbel values (deterministic tests).
 * ------------------------------------------------------------------------------------------ */
/* z~ = sga_round(z_loc, tau); bits[n] = -sum log2 p_DF(z~); sprime = d z~/d z_loc;
 * dbits_dz = d(-log2 p)/d z~ per element. */
int sntc_sga_factorized_fwd(const sntc_prior* prior, const float* z_loc, int n, int64_t hw, float tau,
                            const float* noise, uint64_t seed, uint64_t step, float* z_tilde, float* sprime,
                            float* dbits_dz, double* bits, void* stream);
/* y~ = sga_round(y_loc - mu, tau) + mu with (mu, raw) = hyper halves; bits[n] = -sum log2 p_N(y~ - mu; sigma);
 * sprime = d sga/d u; dbits_dv = d bits/d (y~ - mu); dbits_draw = d bits/d raw (through exp, clamp, SCALE_FN). */
int sntc_sga_normal_fwd(const float* y_loc, const float* hyper, int n, int64_t hw, int c, float tau,
                        const float* noise, uint64_t seed, uint64_t step, float* y_tilde, float* sprime,
                        float* dbits_dv, float* dbits_draw, double* bits, void* stream);
/* g_yloc = (g_ytilde + weight dbits_dv) sprime;  g_hyper = [g_ytilde (1 - sprime) - weight dbits_dv sprime | weight dbits_draw] */
int sntc_sga_normal_bwd(const float* g_ytilde, const float* sprime, const float* dbits_dv, const float* dbits_draw,
                        float weight, int64_t npix, int c, float* g_yloc, float* g_hyper, void* stream);
/* sntc_sga_normal_fwd at one quantisation step per image (mshyper/models.py:285-291 and common/latent_rvs_utils.py:8-48 on the
 * grid of the step; the step rule is that of sntc_step_symbols / sntc_dequant_step above): quant_step float [n] = r^k,
 * inv_step float [n] = r^-k, shift int32 [n] = k, on the device.  Per element, in float32:
 *   u = (y_loc - mu) * inv_step;  (v, sprime) = sga_round(u, tau) and d v / d u;  y~ = fmaf(quant_step, v, mu);
 *   sigma = exp(c0 + c1 clamp(clamp(exp(raw), 0, 63) - k, 0, 63));  bits[n] = -sum log2 p_N(v; sigma);
 *   dbits_dv = d bits / d v;  dbits_draw = d bits / d raw (identity-if-towards on the inner clamp, the plain clamp gradient
 *   on the outer one: zero where the shifted index leaves [0, 63]).
 * Where u is an integer y~ is sntc_dequant_step's value of sntc_step_symbols' symbol.  The Gumbel draw has the keys of
 * sntc_sga_normal_fwd; with quant_step = inv_step = 1.0f, k = 0 the four element-wise outputs are that entry point's, bit for
 * bit.  c % 4 == 0 and 16-byte aligned pointers take 16-byte loads and stores, anything else an element-wise path with the
 * same result.  n <= 65535. */
int sntc_sga_normal_step_fwd(const float* y_loc, const float* hyper, int n, int64_t hw, int c, float tau, const float* noise,
                             uint64_t seed, uint64_t step, const float* quant_step, const float* inv_step, const int32_t* shift,
                             float* y_tilde, float* sprime, float* dbits_dv, float* dbits_draw, double* bits, void* stream);
/* Its backward half (mshyper/models.py:285-291, common/latent_rvs_utils.py:8-48): with a = sprime inv_step, dv = weight dbits_dv,
 * g = g_ytilde dweight[image] (dweight float [n] on the device: the image's weight on the distortion gradient),
 *   g_yloc = (g quant_step + dv) a;  g_hyper = [g (1 - quant_step a) - dv a | weight dbits_draw]
 * -- sntc_sga_normal_bwd's operations at quant_step = inv_step = dweight = 1.0f. */
int sntc_sga_normal_step_bwd(const float* g_ytilde, const float* sprime, const float* dbits_dv, const float* dbits_draw,
                             float weight, int n, int64_t hw, int c, const float* quant_step, const float* inv_step,
                             const float* dweight, float* g_yloc, float* g_hyper, void* stream);
/* sntc_sga_normal_step_fwd with one ladder index per latent POSITION (mshyper/models.py:285-291 and
 * common/latent_rvs_utils.py:8-48 on a grid that varies inside the image; region-of-interest coding, the step rule of
 * sntc_step_map_symbols / sntc_dequant_step_map above): kmap int8 [n][hw] on the device, one index for the c channels of a
 * position, clamped to [-32, 32] before it is used; lut float [2][65] = [step | inv_step] by index + 32 (the table of
 * sntc_step_map_symbols).  At k = kmap[image][position]: u = (y_loc - mu) * lut[1][k + 32], y~ = fmaf(lut[0][k + 32], v, mu), the
 * rate under the table k places down the ladder.  With a map constant per image the four element-wise outputs are
 * sntc_sga_normal_step_fwd's at that index, bit for bit; where u is an integer y~ is sntc_dequant_step_map's value of
 * sntc_step_map_symbols' symbol.  Same Gumbel keys, same 16-byte / element-wise paths.  n <= 65535. */
int sntc_sga_normal_step_map_fwd(const float* y_loc, const float* hyper, int n, int64_t hw, int c, float tau, const float* noise,
                                 uint64_t seed, uint64_t step, const int8_t* kmap, const float* lut, float* y_tilde, float* sprime,
                                 float* dbits_dv, float* dbits_draw, double* bits, void* stream);
/* Its backward half (mshyper/models.py:285-291, common/latent_rvs_utils.py:8-48): with step / inv_step of the position's index,
 * a = sprime inv_step, dv = weight dbits_dv, g = g_ytilde,
 *   g_yloc = (g step + dv) a;  g_hyper = [g (1 - step a) - dv a | weight dbits_draw]
 * -- sntc_sga_normal_step_bwd at dweight = 1.0f: on a map the distortion's weight sits on the pixels
 * (sntc_distortion_grad_weighted), not here. */
int sntc_sga_normal_step_map_bwd(const float* g_ytilde, const float* sprime, const float* dbits_dv, const float* dbits_draw,
                                 float weight, int n, int64_t hw, int c, const int8_t* kmap, const float* lut, float* g_yloc,
                                 float* g_hyper, void* stream);
/* UQLatentRV.sample(training, method, offset, **kwargs) / .quantize(offset) (common/latent_rvs_lib.py:77-116) on [npix, c]
 * values: u = loc - offset (offset NULL = none; else element (p, ch) is offset[p * offset_stride + ch], e.g. the mean half of
 * the hyper-synthesis output with offset_stride = 2 c; offset_stride 0 broadcasts a per-channel [c] offset).  mode 0: round-half-even(u) + offset (training=False, :95-102; also
 * tfc.round_st's forward value, :77-78); 1 'unoise': loc + U(-.5, .5) (:104-107); 2 'sga': sga_round(u, tau = param) + offset
 * (:108-110, common/latent_rvs_utils.py:8-48); 3 'soft_round': tfc.soft_round(u, alpha = param) + offset (:111-114).
 * noise: NULL -> counter-based generator keyed by (seed, step, element); else the uniform values [npix, c] in (-.5, .5) (mode 1)
 * or the Gumbel pairs [npix, c, 2] (mode 2). */
int sntc_uq_sample(const float* loc, const float* offset, int64_t npix, int c, int offset_stride, int mode, float param,
                   const float* noise, uint64_t seed, uint64_t step, float* out, void* stream);
/* out = (g + weight dbits) sprime */
int sntc_sga_chain(const float* g, const float* dbits, const float* sprime, float weight, int64_t total, float* out,
                   void* stream);
/* Training-mode distortion (common/data_lib.py:48-52, no rounding): sse[n] = sum (255 (x - x_hat))^2 over the
 * un-padded h x w region; g_xhat[n,hs,ws,c] = scale (x_hat - x), zero in the padded margin. */
int sntc_distortion_grad(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws, float scale,
                         float* g_xhat, double* sse, void* stream);
/* sntc_distortion_grad with a weight per block x block pixels (common/data_lib.py:48-52; the distortion of SGA on a step map,
 * where the weight varies inside an image and so cannot be applied after the synthesis adjoint): weights float [n][hb][wb] on
 * the device, hb block >= hs and wb block >= ws; pixel (r, s) takes omega = weights[image][r / block][s / block].
 *   g_xhat = (scale omega) (x_hat - x) in the h x w region, zero in the margin;
 *   sse[n] = the UNWEIGHTED sum of (255 (x - x_hat))^2, as sntc_distortion_grad leaves it;  wsse[n] = sum omega (255 (x - x_hat))^2.
 * Both sums are doubles, OVERWRITTEN.  With every weight 1.0f: g_xhat and sse are sntc_distortion_grad's, bit for bit. */
int sntc_distortion_grad_weighted(const float* x, const float* x_hat, int n, int h, int w, int c, int hs, int ws, float scale,
                                  const float* weights, int hb, int wb, int block, float* g_xhat, double* sse, double* wsse,
                                  void* stream);
/* Backward of the activation + residual split of sntc_two_layer_tail: t is the forward input, g_h the gradient
 * w.r.t. h; g_t[npix, cp] = [d act(base) | g_h (if has_res) | zeros up to cp]. */
/* Input gradient of the tail's output layer (Conv2DTranspose 5x5 / 2, ch -> 3, SAME; w2 [5,5,3,ch]):
 * g_h[n, hh, wh, ch] from g_xhat[n, 2 hh, 2 wh, 3] -- an HBM stream, not worth a GEMM launch. */
int sntc_two_layer_out_adjoint(const float* g_xhat, int n, int hh, int wh, int ch, const float* w2, int k2, int s2, int cout,
                               float* g_h, void* stream);
/* abs_x / g_x (both [npix, ch], may both be NULL): |base| and g_h * base, the operands of the IGDN1 parameter
 * gradients of the training step (d gamma = |x|^T (g x) summed over pixels, d beta = column sums of g x). */
int sntc_two_layer_tail_bwd(const float* t, const float* g_h, int64_t npix, int ch, int has_res, int act_kind,
                            const float* beta, const float* gamma, int cp, float* g_t, float* abs_x, float* g_x,
                            void* stream);
/* Keras Adam (tf.keras.optimizers.Adam, no amsgrad) on one flat tensor; t = 1-based step; the gradient is
 * multiplied by grad_scale first (global-norm clipping, optimizer_config.global_clipnorm). */
int sntc_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, int64_t t, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training step: Model.train_step, mshyper/models.py:375-383 = tape.gradient of
 *   frame_loss_given_latent_rvs(training=True) w.r.t. every trainable variable + Adam.
 *   Input gradients are sntc_conv_forward on adjoint plans (see the SGA note above); the pieces below are the
 *   weight / bias gradients, the element-wise backward steps and the training-mode entropy terms.
 * ------------------------------------------------------------------------------------------ */
/* Weight gradient of a Keras-SAME Conv2D (kind SNTC_CONV2D, kernel [kh,kw,cin,cout]) or Conv2DTranspose
 * (SNTC_CONV2D_TRANSPOSE, kernel [kh,kw,cout,cin]) layer, in the layer's own kernel layout:
 *   x      [n,h,w,cin]      the layer input of the forward pass
 *   g_out  [n,ho,wo,cout]   gradient w.r.t. the PRE-activation output (ho = ceil(h/s) or h*s)
 *   dw     written, or accumulated into when accumulate != 0.
 * fp32 MFMA contraction over the pixels, split over blocks, summed in a fixed order (deterministic). */
int64_t sntc_conv_wgrad_workspace_bytes(int kind, int kh, int kw, int stride, int cin, int cout, int n, int h, int w);
int sntc_conv_wgrad(int kind, int kh, int kw, int stride, int cin, int cout, const float* x, const float* g_out, int n,
                    int h, int w, float* dw, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* db[c] (= or +=) sum over pixels of g[npix, c] */
int64_t sntc_bias_grad_workspace_bytes(int64_t npix, int c);
int sntc_bias_grad(const float* g, int64_t npix, int c, float* db, int accumulate, void* workspace, int64_t workspace_bytes,
                   void* stream);
/* g_pre = g * act'(pre) written through the layer output y (relu: y > 0; leaky_relu: 1 or 0.2; sigmoid: y (1 - y)).
 * g_pre may alias g. */
int sntc_act_backward(const float* g, const float* y, int64_t total, int act, float* g_pre, void* stream);
/* SimpleAttention gate unfused (common/elic.py:97-100): out = x + t * s;  g_t = g s, g_spre = g t s (1 - s). */
int sntc_gate_forward(const float* x, const float* t, const float* s, int64_t total, float* out, void* stream);
int sntc_gate_backward(const float* g, const float* t, const float* s, int64_t total, float* g_t, float* g_spre, void* stream);
/* a += alpha * b  (gradient accumulation at fan-outs) */
int sntc_axpy(float* a, const float* b, float alpha, int64_t total, void* stream);
/* out = x + U(-.5, .5): tfc's training=True perturbation (uq method "unoise").  noise NULL -> counter-based
 * generator keyed by (seed, step, element); else float [total] (deterministic tests). */
int sntc_noise_add(const float* x, int64_t total, const float* noise, uint64_t seed, uint64_t step, float* out, void* stream);
/* out[0] (double, device) = sum x^2  (global gradient norm) */
int sntc_sumsq(const float* x, int64_t total, double* out, void* stream);
/* Hidden layer of TwoLayer[Res]Synthesis unfused: h[npix, ch] = act(t[..., :ch]) (+ t[..., ch:2ch]);
 * act_kind as in sntc_two_layer_tail. */
int sntc_two_layer_hidden(const float* t, int64_t npix, int ch, int has_res, int act_kind, const float* beta,
                          const float* gamma, float* h, void* stream);
/* tfc.GDNParameter: eff = max(raw, bound)^2 - pedestal, and its gradient (lower_bound "identity_if_towards"). */
int sntc_gdn_reparam_forward(const float* raw, int64_t total, float bound, float pedestal, float* eff, void* stream);
int sntc_gdn_reparam_backward(const float* raw, const float* g_eff, int64_t total, float bound, float* g_raw, void* stream);
/* Rate terms at a given (noisy) sample: bits[n] = -sum log2 p, d bits / d (y~ - mu), d bits / d raw (normal);
 * d bits / d z~ (deep factorized).  Same formulas as the eval entry points with values_only = 1. */
int sntc_noisy_normal(const float* y_tilde, const float* hyper, int n, int64_t hw, int c, float* dbits_dv,
                      float* dbits_draw, double* bits, void* stream);
/* grad_record (float [sntc_prior_record_floats()], may be NULL): sum over all elements of d bits / d (softplus(matrix),
 * bias, tanh(factor)) per channel, OVERWRITTEN; turn into raw-variable gradients with sntc_prior_param_grad. */
int sntc_noisy_factorized(const sntc_prior* prior, const float* z_tilde, int n, int64_t hw, float* dbits_dz,
                          float* grad_record, double* bits, void* stream);
int sntc_prior_record_floats(const sntc_prior* prior);
/* Refresh the prior from DEVICE arrays of the raw variables (layouts of sntc_prior_create). */
int sntc_prior_update(sntc_prior* prior, const float* matrices, const float* biases, const float* factors, void* stream);
int sntc_prior_param_grad(const sntc_prior* prior, const float* matrices, const float* factors, const float* grad_record,
                          float weight, float* g_matrices, float* g_biases, float* g_factors, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training of the GDN / SignalConv2D stacks (MBT2018*, BLS2017*: reference common/transforms.py:93-175 under
 * Model.train_step, mshyper/models.py:375-383).  GDN with alpha = 1, epsilon = 1 (the reference's GDN1, :8-63):
 * norm = beta + |x| gamma comes from a 1x1 convolution plan with the |x| prologue; these are the element-wise parts.
 *   sntc_gdn_apply:            y = x / norm (inverse: x * norm)
 *   sntc_gdn_backward_prep:    q = d loss / d norm = -g x / norm^2 (inverse: g x);  abs_x = |x|
 *   sntc_gdn_backward_finish:  dx = g / norm (inverse: g * norm) + sign(x) * t,  t = q gamma^T from the adjoint 1x1 plan
 * d beta = column sums of q (sntc_bias_grad), d gamma = |x|^T q (sntc_conv_wgrad, 1x1).
 * ------------------------------------------------------------------------------------------ */
int sntc_gdn_apply(const float* x, const float* norm, int64_t total, int inverse, float* y, void* stream);
int sntc_gdn_backward_prep(const float* g, const float* x, const float* norm, int64_t total, int inverse, float* q, float* abs_x,
                           void* stream);
int sntc_gdn_backward_finish(const float* g, const float* x, const float* norm, const float* t, int64_t total, int inverse,
                             float* dx, void* stream);
/* out[rows, cols] = a[rows, k] b[k, cols] (transpose_a: a is [k, rows]) for a small left matrix (<= 48 KB): the
 * tfc.RDFTParameter of SignalConv2D kernels (transforms.py:101-112), kernel = M rdft and d rdft = M^T d kernel. */
int sntc_small_matmul(const float* a, const float* b, int rows, int k, int64_t cols, int transpose_a, float* out, void* stream);
/* dst[t, b, a] = src[t, a, b]: sntc_conv_wgrad of a SNTC_SIGNAL_UP layer returns [kh, kw, Cout, Cin]; its kernel is
 * [kh, kw, Cin, Cout] (tfc.SignalConv2D, transforms.py:123-134,172-175). */
int sntc_transpose_last2(const float* src, int taps, int a, int b, float* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SNTC_H_ */
