/* libyolo2_hip.so -- C ABI of the MI355X (gfx950) Darknet-19 / YOLO grid-detector path.
 *
 * The reference (wenxichen/tensorflow_yolo2) has no FFI: its boundary is a set of
 * Python functions that build TF1 graph nodes.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  The
 * Python mirrors of those functions (tensorflow_yolo2_amd/yolo2_nets/) bind
 * these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions: plain C types only; every function returns 0 on success or a
 * negative error code (message: y2_last_error()); the CALLER owns every device
 * buffer (parameters, gradients, BN state, workspace, inputs, outputs); no hidden
 * device allocation; all work is enqueued on the hipStream_t passed as `stream`
 * (void*, NULL = default stream) and is asynchronous w.r.t. the host; one context
 * per thread/device (thread-compatible, not thread-safe).
 * Tensors are NHWC fp32 at the boundary (as the reference feeds TF); filters HWIO.
 */
#ifndef YOLO2_HIP_H
#define YOLO2_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the declarations below are exported */
#pragma GCC visibility push(default)

typedef struct y2_ctx y2_ctx;

/* arithmetic type of the MFMA contractions / stored activations */
#define Y2_F32 0  /* exact-f32 MFMA (v_mfma_f32_32x32x2_f32): parity mode        */
#define Y2_F16 1  /* fp16 operands, fp32 accumulate                              */
#define Y2_BF16 2 /* bf16 operands, fp32 accumulate                              */
/* Round 5: the reference's precision on the FAST matrix pipe.  The reference is fp32 end to end
 * (src/yolo2_nets/darknet.py:10-46, tf.float32 placeholders src/pascal/pascal_train_darknet.py:34-36).  Every MFMA
 * operand (activation, filter, dY) is a pair of halves hi = f16(v), lo = f16(v - hi) in two planes of its channel row
 * (4 bytes per element, as fp32); a product is hi*hi + lo*hi + hi*lo on v_mfma_f32_*_f16 with fp32 accumulation
 * (~22 mantissa bits, a third of the f16 rate instead of the exact-f32 MFMA's sixteenth); conv outputs, gradients
 * with respect to activations, statistics, batch norm, loss and optimizer are fp32 as in Y2_F32; the 3-channel image
 * layer runs in exact fp32.  Gradients ride on the f16 loss scale (y2_set_options) with the f16 mode's overflow guard.
 * Range: the filter planes hold 64 * w in f16 (a power-of-two pre-scale that keeps typical weights' lo plane out of the
 * subnormals), so |w| must stay below 1024; activations and dY have f16's range. */
#define Y2_F16X2 3
/* Round 6: Y2_F16X2 forward, single-product backward.  Tensors, forward pass, batch norm, loss and optimizer are exactly
 * Y2_F16X2's (so every forward DECISION -- leaky branch, pool arg-max, responsible box -- is the reference-precision one);
 * the two backward contractions of tf.gradients (Conv2DBackpropInput / Conv2DBackpropFilter behind
 * src/pascal/pascal_train_darknet.py:49-51) read the hi planes of dY, W and x only: one f16 MFMA per product with fp32
 * accumulation.  With the decisions fixed the backward pass is linear in dY, so the f16 operand rounding (2^-11 relative
 * per element, random) is not amplified: gradients stay within the 1e-3 tolerance of the whole-step gates
 * (tests/test_gpu_f16x2f.py), at roughly a third of the backward cost of Y2_F16X2.  y2_ctx_create and the op-level
 * y2_conv2d / y2_conv2d_backward accept it. */
#define Y2_F16X2F 4
/* MXFP8 inference (OCP MX spec): the forward convolutions of the layers whose batch norm uses the moving statistics and
 * whose shape measured no slower than f16 run on gfx950's block-scaled matrix pipe
 * (v_mfma_scale_f32_32x32x64_f8f6f4, twice the f16 rate per clock) with fp32 accumulation.  Elements are OCP e4m3fn (not the fnuz encoding); each block of 32 values shares one E8M0 scale byte
 * (2^(byte - 127)).  A block is 32 consecutive channels of one pixel (activations, NHWC) or 32 consecutive input channels
 * of one tap and one output channel (filters, HWIO).  Scale of a block: the smallest e with amax <= 448 * 2^e -- with
 * frexp(amax) = m * 2^E, e = E - 9 if m <= 0.875 else E - 8 -- clamped to [-127, 127]; an all-zero block takes -127.
 * Elements: round-to-nearest-even e4m3 of v / 2^e (clamped to +-448 as a guard; subnormals kept).  Every other layer --
 * the 3-channel image layer, layers with batch statistics -- runs exactly as in Y2_F16, whose tensors (f16) the mode
 * stores.  Inference only: y2_bind(training = 1), the y2_backward* family and y2_conv2d_backward refuse it.
 * y2_conv2d accepts it (fp32 x / w in, both quantised in the workspace, fp32 y out; Cin % 32 == 0). */
#define Y2_FP8 5

#define Y2_TAIL_NONE 0    /* output = last layer activation [N,Ho,Wo,Cout]       */
#define Y2_TAIL_AVGPOOL 1 /* + average_pooling2d(k,k) + reshape -> [N,Cout]      */

#define Y2_OK 0
#define Y2_ERR_ARG -1
#define Y2_ERR_HIP -2
#define Y2_ERR_STATE -3

const char* y2_last_error(void);
int y2_version(void);

/* Layer list of the reference networks, 4 ints per layer (filter_size, in_chl,
 * out_chl, maxpool_after).  kind 0: darknet19_core (src/yolo2_nets/darknet.py:126-179),
 * kind 1: core + darknet19_detection(output_filter) (darknet.py:182-201),
 * kind 2: darknet19 classifier (darknet.py:61-123).  Returns the layer count. */
int y2_darknet19_spec(int kind, int output_filter, int* spec, int max_layers);

/* ---- network context (replaces the TF graph + variables built by
 *      conv_bn_layer, src/yolo2_nets/darknet.py:32-46) ------------------------
 * spec: 4 ints per layer (filter_size, in_chl, out_chl, after).  after = 0: nothing; 1: tf.nn.max_pool(2, 2, 'SAME')
 * behind the activation (darknet.py:24-25,45); 2 (round 5, inner layers on even maps): SUBSAMPLE -- the layer is slim's
 * conv2d_same(stride=2) / subsample (src/slim_dir/nets/resnet_utils.py:60-122): its stride-1 output at even rows and
 * columns, batch norm over those positions only (the 3x3 convolution of a stride-2 bottleneck unit, resnet_v1.py:99-112) */
int y2_ctx_create(y2_ctx** out, const int* spec, int num_layers, int core_layers, int tail, int tail_k,
                  int batch, int height, int width, int dtype);
void y2_ctx_destroy(y2_ctx* ctx);
/* A GROUP of bound contexts on one flat parameter buffer (round 5: the 20 stacks of the ResNet swap) re-packs its filters
 * in ONE launch instead of one per context.  y2_pack_group_table: once, outside any stream capture (a synchronous copy) --
 * the concatenated pack tables into caller-owned device memory (table_bytes >= 128 * layers is ample); returns the layer
 * and block counts.  y2_pack_group_run: the launch; afterwards the contexts' packed copies are current (the lazy pack of
 * their next y2_forward is skipped).  Contexts with a 3-channel first layer pack on their own. */
int y2_pack_group_table(y2_ctx** ctxs, int n, void* table_dev, size_t table_bytes, int* nlayers, int* blocks);
int y2_pack_group_run(y2_ctx** ctxs, int n, const void* table_dev, int nlayers, int blocks, void* stream);
int y2_num_layers(const y2_ctx* ctx);
/* info: k, cin, cout, pool, H, W (conv input = output spatial size), Ho, Wo */
int y2_layer_info(const y2_ctx* ctx, int layer, int info[8]);
/* trainable floats in reference creation order per layer: W (HWIO), b, gamma, beta */
size_t y2_param_count(const y2_ctx* ctx);
/* BN moving statistics per layer: moving_mean, moving_variance */
size_t y2_state_count(const y2_ctx* ctx);
/* off[0..3]: W, b, gamma, beta offsets (floats) into params/grads; off[4..5]: moving_mean, moving_variance into state */
int y2_param_offsets(const y2_ctx* ctx, int layer, size_t off[6]);
int y2_output_shape(const y2_ctx* ctx, int shape[4]);
size_t y2_workspace_bytes(const y2_ctx* ctx, int training);
int y2_bind(y2_ctx* ctx, float* params, float* grads, float* state, void* workspace, size_t workspace_bytes,
            int training, void* stream);
/* loss-scale applied to half-precision gradients (1 = none); moving-variance Bessel switch */
int y2_set_options(y2_ctx* ctx, float grad_scale, int bessel_moving_var);
/* Round 4.  Per-layer activation slopes (max(slope*z, z): 0.1 = the reference's leaky ReLU, src/yolo2_nets/darknet.py:5,45;
 * 0 = ReLU, 1 = no activation) and the batch-norm constants of the stack (defaults: tf.layers.batch_normalization's
 * eps 1e-3 / momentum 0.99, darknet.py:39-44).  For stacks that restate slim's resnet_v1 bottleneck
 * (src/slim_dir/nets/resnet_v1.py:99-112; arg scope src/slim_dir/nets/resnet_utils.py:230-257: conv2d without bias +
 * batch_norm(decay 0.997, epsilon 1e-5) + ReLU, the unit's last conv without activation): slopes {0, 0, 1}, eps 1e-5,
 * momentum 0.997, zero_bias_grad = 1 (the bias slots stay in the flat parameter layout; the caller keeps them at zero
 * and they receive no gradient).  slopes == NULL keeps the current slopes; the 3-channel image layer only takes 0.1. */
int y2_set_layer_options(y2_ctx* ctx, const float* slopes, int num_layers, float bn_eps, float bn_momentum,
                         int zero_bias_grad);
/* weight_variable / bias_variable / BN initial values (darknet.py:10-17): truncated
 * normal(0.1) re-drawn beyond 2 sigma, 0.1, gamma 1, beta 0, moving 0 / 1 */
int y2_init_params(y2_ctx* ctx, uint64_t seed, void* stream);
/* call after params were changed from outside (load / optimizer on a foreign buffer) */
int y2_params_changed(y2_ctx* ctx);

/* darknet19_core / darknet19_detection / darknet19 forward
 * (darknet.py:61-201): images [N,H,W,3] fp32 -> out (shape: y2_output_shape) */
/* update_moving: apply the momentum-0.99 moving-statistics update of the training-mode layers inside this
 * forward (the train step); 0 = leave them alone, as a TF run that does not fetch train_op / UPDATE_OPS does
 * (pascal_detect_darknet.py:61: the head's default is_training=True normalises with batch statistics at
 * detect time, but nothing updates).  y2_update_moving_stats applies the skipped update afterwards, once. */
int y2_forward(y2_ctx* ctx, const float* images, int is_training_core, int is_training_head, int update_moving,
               float* out, void* stream);
/* Round 4.  The stack as the residual branch of a bottleneck unit (src/slim_dir/nets/resnet_v1.py:99-112: output =
 * tf.nn.relu(shortcut + residual)): out = max(join + stack(images), 0), join [like out] fp32 -- the values of y2_forward
 * followed by y2_add_relu, bit for bit; the branch output is never stored.  y2_backward* then takes
 * y2_add_relu_backward's result (the gradient of the branch output), as after the two-call form. */
int y2_forward_join(y2_ctx* ctx, const float* images, const float* join, int is_training_core, int is_training_head,
                    int update_moving, float* out, void* stream);
/* y2_forward fed with what image_read holds BEFORE its float conversion (src/img_dataset/pascal_voc.py:60-67:
 * cv2.imread + cv2.resize give uint8 BGR): images_u8 [N,H,W,3] uint8; the conversion
 * image.astype(float32) / 255.0 * 2.0 - 1.0 (pascal_voc.py:63-64, same fp32 operation order) runs inside the
 * input pack kernel -- a fed training loop uploads 1 byte per value instead of 4. */
int y2_forward_u8(y2_ctx* ctx, const uint8_t* images_u8, int is_training_core, int is_training_head,
                  int update_moving, float* out, void* stream);
int y2_update_moving_stats(y2_ctx* ctx, void* stream);
/* TF autodiff of the stack (tf.train.*Optimizer().minimize, pascal_train_darknet.py:49-51):
 * dout has the output's shape; gradients are written to the bound `grads` buffer
 * for layers [layer_lo, layer_hi) walking downwards; call with (0, num_layers)
 * for the whole net, or in slices to overlap the all-reduce of finished layers. */
int y2_backward(y2_ctx* ctx, const float* dout, int layer_lo, int layer_hi, void* stream);
/* All layers in one pass, with an event pair recorded when every layer >= mark_layers[k] is complete (data
 * parallelism: the all-reduce of a gradient slice starts behind y2_wait_mark on its own stream while the
 * pass continues; no join on `stream` until the end, unlike one y2_backward call per slice). */
int y2_backward_marks(y2_ctx* ctx, const float* dout, int n_marks, const int* mark_layers, void* stream);
int y2_wait_mark(y2_ctx* ctx, int k, void* stream);
/* y2_backward over all layers that also writes the gradient with respect to the stack's input, fp32 NHWC
 * [N,H,W,in_chl of layer 0]: for stacks composed into larger graphs (the YOLOv2 detector of the north star: 13x13
 * stack and head behind the passthrough concat).  The 3-channel image layer has no input gradient. */
int y2_backward_input(y2_ctx* ctx, const float* dout, float* dinput, void* stream);
/* copy a layer's saved activation for tests.  what: 0 = bordered input of `layer` (post BN+leaky+pool of the layer
 * below) [N,H,W,in_chl]; 1 = conv output [N,H,W,out_chl]; 2 = dy * grad_scale [N,H,W,out_chl]; 3 = the per-channel
 * constants the last forward normalised the layer with, [4][out_chl]: mean, 1/sqrt(var + eps), scale, shift */
int y2_debug_read(y2_ctx* ctx, int layer, int what, float* dst, void* stream);

/* Optional measurement aid: bracket every kernel launch of y2_forward / y2_backward with
 * HIP events on the launch stream (the reference only has utils/timer.py wall clocks).
 * Categories: 0 conv fwd (implicit GEMM), 1 conv1 fwd, 2 dgrad, 3 wgrad, 4 conv1 wgrad,
 * 5 BN fwd passes, 6 BN bwd passes, 7 pack/convert.  on = 1: every launch, serialised
 * (no side stream); on = 2: only the MFMA convolution launches (categories 0, 2, 3), streams as in production;
 * on = 0 stops recording but keeps the records, on = 3 resumes mode 2 without clearing (sampling some steps).  collect() waits for the events. */
int y2_profile_enable(y2_ctx* ctx, int on);
int y2_profile_collect(y2_ctx* ctx, double* ms_by_category, int* launches_by_category, int ncat);
/* length of the union of the [start, end] intervals of the launches whose category bit is set in cat_mask
 * (weight gradients run on a side stream beside the dgrads: summing durations would count shared time twice).
 * Call before y2_profile_collect (which resets). */
int y2_profile_busy(y2_ctx* ctx, int cat_mask, double* busy_ms, int* launches);
/* ms[num_layers][8]: the same records per layer and category (does not reset) */
int y2_profile_layers(y2_ctx* ctx, double* ms);

/* ---- get_loss / get_iou / show_yolo_detection (src/yolo2_nets/net_utils.py:222-439) */
size_t y2_yolo_loss_workspace_bytes(int batch, int S);
/* loss[5] = class, object, noobject, coord, total; dnet may be NULL */
int y2_yolo_loss(const float* net, const float* labels, int num_class, int batch, float image_size, int S, int B,
                 float lambda_coord, float lambda_noobj, float* loss, float* ious, float* object_mask,
                 float* dnet, void* workspace, void* stream);
int y2_get_iou(const float* boxes1, const float* boxes2, float* iou, int n_boxes, void* stream);
/* det[(cell*B+b)*8 + {keep, upper_left_x, upper_left_y, w, h, class, cell_row, cell_col}] */
int y2_decode_detections(const float* predict, int S, int B, int num_class, int im_w, int im_h,
                         float object_thresh, int* det, float* conf, void* stream);
/* sparse_softmax_cross_entropy_with_logits + reduce_mean (imagenet_train_darknet.py:51-53) */
int y2_softmax_cross_entropy(const float* logits, const int* labels, int batch, int classes, float* loss,
                             float* dlogits, void* stream);

/* accuracy = reduce_mean(cast(equal(argmax(logits, 1), labels))) (imagenet_train_darknet.py:60-61; ties: the
 * smallest index, as tf.argmax) */
int y2_accuracy(const float* logits, const int* labels, int batch, int classes, float* accuracy, void* stream);

/* ---- YOLOv2 pieces named by the north star that the reference does NOT contain (SURVEY §8 a-x1, a-x2):
 *      no reference interface to cite; specification = oracle/ext_ref.py of this repo. ------------- */
/* standalone tf.nn.max_pool(2, 2, 'SAME') on fp32 NHWC (reference darknet.py:24-25) and its gradient (first
 * maximum in row-major window order); the executor pools inside its BN pass, composed graphs use this op */
int y2_maxpool2x2(const float* x, float* y, int N, int H, int W, int C, void* stream);
int y2_maxpool2x2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* reorg / space-to-depth: forward x [N,H,W,C] -> y [N,H/s,W/s,s*s*C], channel ((h%s)*s + w%s)*C + c;
 * forward = 0: the inverse permutation (x coarse -> y [N,H,W,C]), i.e. the gradient.  Bit-exact copies. */
int y2_reorg(const float* x, float* y, int N, int H, int W, int C, int stride, int forward, void* stream);
/* passthrough: out [N,H,W,4*Cf+Cc] = concat(reorg2(fine [N,2H,2W,Cf]), coarse [N,H,W,Cc]) and its gradient */
int y2_passthrough_concat(const float* fine, const float* coarse, float* out, int N, int H, int W, int Cf, int Cc,
                          void* stream);
int y2_passthrough_concat_backward(const float* dout, float* dfine, float* dcoarse, int N, int H, int W, int Cf,
                                   int Cc, void* stream);
/* Darknet's passthrough, forward (specification: utils/darknet_reorg.py): out [N,H,W,4*Cf+Cc] = Darknet's `reorg`
 * (stride 2, as yolov2-voc.cfg runs it: a scramble of each image over channels and positions, not a space-to-depth) of
 * fine [N,2H,2W,Cf] in channels 0 .. 4*Cf-1, coarse [N,H,W,Cc] behind it -- `route layers=-1,-4`.  A pure gather, bit
 * exact, one launch.  Y2_ERR_ARG: a null tensor, a size below 1, Cf % 4 != 0, an image beyond 32-bit indices. */
int y2_passthrough_concat_darknet(const float* fine, const float* coarse, float* out, int N, int H, int W, int Cf, int Cc,
                                  void* stream);
/* Its gradient (specification: utils/darknet_reorg.passthrough_concat_darknet_backward): dout [N,H,W,4*Cf+Cc] ->
 * dfine [N,2H,2W,Cf] (the inverse of Darknet's reorg, a permutation of each image) and dcoarse [N,H,W,Cc].  One launch
 * writes every element of both outputs exactly once: no zero fill, no atomics, bit exact.  Y2_ERR_ARG as above. */
int y2_passthrough_concat_darknet_backward(const float* dout, float* dfine, float* dcoarse, int N, int H, int W, int Cf,
                                           int Cc, void* stream);
/* Darknet's `[maxpool] size=2 stride=1` on fp32 NHWC (specification: utils/darknet_maxpool.py): y [N,H,W,C], y(i, j) =
 * the maximum of x(i + dy, j + dx), dy, dx in {0, 1}, over the taps inside the map -- a window anchored top-left and
 * clipped at the bottom and right edges; the maximum starts at -FLT_MAX and moves on a strict >, so the first maximum
 * wins a tie and a NaN is never chosen.  Bit exact, one launch; 16-byte accesses when C % 4 == 0 and the pointers are
 * 16-byte aligned, one float per lane otherwise.  Y2_ERR_ARG: a null tensor, a size below 1, more than 2^31 - 1 elements. */
int y2_maxpool2x2s1(const float* x, float* y, int N, int H, int W, int C, void* stream);
/* Its gradient: dx(p) = the float32 sum, from +0, of the dy of the up to four windows whose arg-max p is, in ascending
 * row-major order of their anchors.  A gather: every dx element is written exactly once, no zero fill, no atomics, the
 * same bits every run; a window of NaNs alone routes no gradient.  Y2_ERR_ARG as above. */
int y2_maxpool2x2s1_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* x[0 .. n) = 0 on an fp32 buffer (a trainer's gradient masks: parameters that must not move) */
int y2_zero(float* x, size_t n, void* stream);
/* Darknet's network input from uint8 BGR pixels: dst[p][c] = float(src[p][2 - c]) / 255.0f (RGB in [0, 1]; a true
 * division, bit-equal to numpy's float32 quotient).  Y2_ERR_ARG: a null tensor, n_pixels = 0. */
int y2_u8_bgr_to_f32_rgb(const uint8_t* src, float* dst, size_t n_pixels, void* stream);
/* dst += src on fp32 buffers: the gradient of a tensor with two consumers (the 26x26x512 activation feeds the pool
 * and the passthrough) */
int y2_accumulate(float* dst, const float* src, size_t n, void* stream);
/* Round 4.  The join of a bottleneck unit, output = tf.nn.relu(shortcut + residual) (src/slim_dir/nets/resnet_v1.py:112),
 * and its backward g = (dout + dout2) * [out > 0] (the gradient of both addends; dout2 nullable: the incoming gradient
 * as the two branch gradients of the unit above, never summed in memory); fp32 tensors of n elements, 16-byte aligned. */
int y2_add_relu(const float* a, const float* b, float* out, size_t n, void* stream);
int y2_add_relu_backward(const float* dout, const float* dout2, const float* out, float* g, size_t n, void* stream);
/* Round 5.  LINKED stacks: the stride-1 bottleneck units of the ResNet swap (src/slim_dir/nets/resnet_v1.py:99-112;
 * src/pascal/pascal_train_resnet.py:37-50) hand activations and gradients to each other in the arithmetic type instead of
 * through fp32 NHWC tensors (round 4: a cast, a pack and a convert pass on both sides of every join).
 *   y2_bordered_bytes: size of a zero-bordered tensor [N][H+1][W+1][C] of `dtype` with its guard bands, and the byte
 *     offset of cell 0 inside it; the caller allocates it ZEROED once (borders and guards are never written).
 *   y2_link: tensors of the NEXT y2_forward / y2_backward calls of this context (all nullable; pointers address cell 0):
 *     x_bordered   layer 0's input is this tensor (y2_forward's `images` may then be NULL; no pack pass)
 *     out_bordered the last layer's activation is written here (the consumer's input; y2_forward's `out` may be NULL)
 *     join_bordered / join_self   the stored value is relu(join + stack(x)) with the join read from a bordered tensor of
 *                  the output's geometry, or from the stack's own layer-0 input (identity shortcut); either output form
 *     dout_t       [M][out_chl] of T: d loss / d (pre-join output) * grad_scale (y2_backward's `dout` may be NULL)
 *     dx_t         [M][in_chl] of T: receives d loss / d input * grad_scale (beside, or instead of, y2_backward_input's fp32)
 *   y2_join_backward: g = (d1 + d2) * [out > 0], all of T except d2 when d2_f32 (the g of a run's top unit, fp32);
 *     out bordered (the unit's output as its consumer holds it), d1 / d2 / g [M][C]. */
size_t y2_bordered_bytes(int N, int H, int W, int C, int dtype, size_t* cell0_offset);
int y2_link(y2_ctx* ctx, void* x_bordered, void* out_bordered, const void* join_bordered, int join_self, const void* dout_t,
            void* dx_t);
int y2_join_backward(int dtype, const void* out_bordered, const void* d1, const void* d2, int d2_f32, void* g, int N, int H,
                     int W, int C, void* stream);
/* ... with a STRIDE-2 unit above (round 5: the last unit of blocks 1-3 inside a linked run).  y2_subsample_bordered:
 * resnet_utils.subsample(x, 2) (resnet_utils.py:60-75) from a bordered tensor [N][H+1][W+1][C] of T into one of half the
 * size -- that unit's identity shortcut, joined in its last apply pass (y2_link join_bordered).  y2_join_backward_s2: as
 * y2_join_backward, but d2 -- the gradient of that shortcut -- lives on the upper unit's OUTPUT grid [N*H/2*W/2][C] and
 * reaches the even rows / columns of this [N*H*W] grid only. */
int y2_subsample_bordered(int dtype, const void* src_bordered, void* dst_bordered, int N, int H, int W, int C, void* stream);
int y2_join_backward_s2(int dtype, const void* out_bordered, const void* d1, const void* d2, int d2_f32, void* g, int N, int H,
                        int W, int C, void* stream);
/* scores [rows][classes] -> best score and class index per row (the class choice in front of the NMS of the YOLOv2
 * detector; ties: smallest index, as np.argmax in net_utils.py:418) */
int y2_class_argmax(const float* scores, float* best, int* cls, int rows, int classes, void* stream);
/* x *= s: the loss scale in front of a half-precision backward pass of a composed graph (no reference counterpart:
 * the reference runs fp32) */
int y2_scale(float* x, size_t n, float s, void* stream);
/* anchor decode: net [N,S,S,B,5+C] (tx,ty,tw,th,to,classes), anchors [B][2] in cell units ->
 * boxes [N,S*S*B,4] (cx,cy,w,h relative to the image), scores [N,S*S*B,C] = sigmoid(to)*softmax(classes) */
int y2_decode_anchors(const float* net, const float* anchors, float* boxes, float* scores, int N, int S, int B, int C,
                      void* stream);
/* per-image greedy NMS over K <= 4096 candidates: score descending (ties: lower index first), candidates
 * below score_thresh dropped, a kept box suppresses later boxes with IoU > iou_thresh (same class id only
 * when class_aware).  keep [N][max_out] original indices (-1 padded), count [N].  Bit-exact vs the spec. */
int y2_nms(const float* boxes, const float* scores, const int* classes, int N, int K, float iou_thresh,
           float score_thresh, int max_out, int class_aware, int* keep, int* count, void* stream);

/* YOLOv2 anchor-box loss, forward + gradient (specification: oracle/ext_ref.py yolov2_loss): net [N,S,S,B,5+C]
 * raw outputs, labels = the reference's label grid [N,S,S,5+C] (one box per cell, img_dataset/pascal_voc.py:146-163),
 * anchors [B][2] in cell units, scales = {coord, object, noobject, class, iou_thresh} (NULL: 1, 5, 1, 1, 0.6).
 * loss[5] = coord, object, noobject, class, total (mean over the batch); dnet (nullable) same shape as net. */
size_t y2_yolov2_loss_workspace_bytes(int batch);
int y2_yolov2_loss(const float* net, const float* labels, const float* anchors, int batch, int S, int B, int num_class,
                   float image_size, const float* scales, float* loss, float* dnet, void* workspace, void* stream);
/* The same loss on BOX LISTS, every object of an image kept (specification: utils/region_loss.py yolov2_loss_boxes):
 * truth [N][max_boxes][5] = cx, cy, w, h in pixels of the input and the class index, ntruth int32 [N] (y2_encode_box_list
 * writes both; device memory).  The loss derives a truth's cell and its best-fitting anchor; the slot (cell, anchor) is
 * owned by the LOWEST truth index that claims it, a truth that loses its slot has no coord / object / class term but
 * still counts in the best IoU of the noobject rule.  `scales`: 7 floats in HOST memory = {coord, object, noobject,
 * class, iou_thresh, area_weight (0 / 1: coord terms times 2 - w h, w and h relative to the image), prior_scale (> 0:
 * every un-owned slot adds prior_scale ((sig(tx) - 1/2)^2 + (sig(ty) - 1/2)^2 + tw^2 + th^2) to the coord part)}; NULL:
 * 1, 5, 1, 1, 0.6, 0, 0.  One launch + the finalize; the result does not vary from run to run.  The ownership table is
 * held in LDS in slices of 256 slots, one per workgroup, so S * S * B is bounded by the index arithmetic alone
 * (Y2_LOSS_BOXES_MAX_SLOTS).  A class index outside [0, num_class) is the caller's error: the lists are device memory,
 * no host-side check is made, and such a row takes no class term (its other terms stand). */
#define Y2_LOSS_BOXES_MAX_SLOTS (1 << 20) /* S * S * B of one image; more is an argument error */
size_t y2_yolov2_loss_boxes_workspace_bytes(int batch, int S, int B);
int y2_yolov2_loss_boxes(const float* net, const float* truth, const int* ntruth, const float* anchors, int batch, int S,
                         int B, int num_class, int max_boxes, float image_size, const float* scales, float* loss,
                         float* dnet, void* workspace, void* stream);
/* Region statistics of the same inputs (specification: utils/region_loss.py region_stats_boxes): the numbers of Darknet's
 * region-layer log line.  Every listed truth counts, owner of its slot or not (Darknet's layer has no ownership rule);
 * per truth the prediction at its cell and best-fitting anchor is decoded.  stats[6] in device memory = mean IoU, mean
 * softmax probability of the true class (over the truths whose class lies in [0, num_class)), mean sig(to) at the truths,
 * mean sig(to) over all batch * S * S * B slots, share of truths with IoU > 0.5, truth count.  A mean over nothing is 0.
 * One launch (a workgroup per image) + the finalize; no atomics: the result does not vary from run to run.  Argument
 * errors are the loss entry's, and B <= 8. */
size_t y2_yolov2_region_stats_workspace_bytes(int batch);
int y2_yolov2_region_stats(const float* net, const float* truth, const int* ntruth, const float* anchors, int batch, int S,
                           int B, int num_class, int max_boxes, float image_size, float* stats, void* workspace,
                           void* stream);

/* ---- The word tree of the region layer (YOLO9000's softmax_tree; specification: utils/word_tree.py; csrc/word_tree.hip).
 *      The class logits of a head row are the nodes of a tree: a softmax per group of siblings, abs[node] = the product
 *      of the conditionals on the node's path to a root.  `tables`: device memory, int32 [3 num_class + 2 G] =
 *      parent[num_class], group[num_class], child[num_class], group_offset[G], group_size[G], as utils/word_tree.py
 *      pack() writes them; G the group count, max_depth the largest node depth (a root has depth 0).  The host cannot
 *      check the content of device tables: the kernels cut every value they read from them into its range and bound
 *      every walk by max_depth + 1 levels, so no table and no truth list makes them read or write outside a head row or
 *      a table, or spin; with tables pack() did not write the results are unspecified.  Argument errors of all three
 *      entries, nothing launched, named with the entry and the item: a null pointer, num_class outside
 *      1..Y2_WORD_TREE_MAX_NODES, G outside 1..num_class, max_depth outside 0..num_class - 1. ------------------------- */
#define Y2_WORD_TREE_MAX_NODES 65536 /* num_class with a tree; the kernels hold no node in LDS, so this bounds index
                                        arithmetic only (the executor's 2,048-column row allows 404 at B = 5) */
/* y2_yolov2_loss_boxes with the class term of the word tree (specification: utils/word_tree.py yolov2_loss_boxes_tree):
 * cells, best anchor, ownership, the coord / object / noobject parts, `scales`, loss[5], dnet and the workspace are that
 * entry's, with its argument errors.  An owned slot whose class k lies in [0, num_class) takes, for each node a of k,
 * parent[k], ... up to a root (at most max_depth + 1 nodes) with g = group[a], class_scale (lse_g - logit[a]) into the
 * class part and class_scale (softmax_g - onehot(a)) / batch into the gradient of g's members; every other class entry
 * of dnet is 0.  Any node may be a truth, an inner one too.  A class index outside [0, num_class) takes no class term.
 * Every gradient row is written with consecutive lanes on consecutive floats; partial sums are added in a fixed order:
 * the result does not vary from run to run.  One launch + the finalize. */
size_t y2_yolov2_loss_boxes_tree_workspace_bytes(int batch, int S, int B);
int y2_yolov2_loss_boxes_tree(const float* net, const float* truth, const int* ntruth, const float* anchors,
                              const int* tables, int batch, int S, int B, int num_class, int G, int max_depth,
                              int max_boxes, float image_size, const float* scales, float* loss, float* dnet,
                              void* workspace, void* stream);
/* y2_yolov2_region_stats with stats[1] = the mean of abs[class] over the truths whose class lies in [0, num_class)
 * (specification: utils/word_tree.py region_stats_boxes_tree; Darknet's avg_cat).  Everything else, the workspace
 * (y2_yolov2_region_stats_workspace_bytes) and the argument errors are that entry's. */
int y2_yolov2_region_stats_tree(const float* net, const float* truth, const int* ntruth, const float* anchors,
                                const int* tables, int batch, int S, int B, int num_class, int G, int max_depth,
                                int max_boxes, float image_size, float* stats, void* workspace, void* stream);
/* The detection head of a tree (specification: utils/word_tree.py word_tree_head): net [rows][5 + num_class], rows =
 * batch * S * S * B -> out of the same shape: elements 0..4 bit-identical copies, the class logits replaced by 0.0f at
 * `top` and -inf everywhere else.  top: start at the root group with p = 1; j = the first maximum of the group; while
 * p cond[j] > tree_thresh take it (p *= cond[j]) and go on in j's child group, j itself where it is a leaf; where the
 * product does not pass, the answer is the node taken last -- or j, with p = cond[j], in the root group, which always
 * answers.  Optional outputs (NULL: not written): top int32 [rows], prob [rows] = abs[top], multiplied root first.
 * out == net (in place) is allowed and gives the same bits.  Every detect entry reads such a row unchanged and exactly:
 * its softmax finds maximum 0 and sum 1, so the score is sig(to) at top and 0 elsewhere.  One launch, a wave per row.
 * Y2_ERR_ARG also: rows < 1, tree_thresh outside [0, 1). */
int y2_word_tree_head(const float* net, const int* tables, int rows, int num_class, int G, int max_depth,
                      float tree_thresh, float* out, int* top, float* prob, void* stream);
/* The walk of y2_word_tree_head without the rewrite (csrc/detect_tree.hip): net is read only and no row is written; top
 * (required) and prob (NULL: not written) are bit for bit what y2_word_tree_head writes for the same row.
 * obj_thresh < 0: every row is walked.  obj_thresh >= 0: a row whose objectness so = 1 / (1 + expf(-net[row][4])) -- the
 * float32 expression of y2_decode_anchors -- is not > obj_thresh (NaN included) gets top = -1, prob = 0, and none of its
 * class logits is read: on a trained head that is nearly every row.  One launch, a wave per row, no LDS.
 * Y2_ERR_ARG: y2_word_tree_head's, a null top, an obj_thresh that is not finite. */
int y2_word_tree_top(const float* net, const int* tables, int rows, int num_class, int G, int max_depth,
                     float tree_thresh, float obj_thresh, int* top, float* prob, void* stream);

/* ---- The wide head (csrc/wide_head.hip): a 1x1 convolution wider than the executor's 2,048-column row -- YOLO9000's last
 *      layer, 1024 -> 28,269 -- as an operator behind the head stack (its gradients and its update: the section below).
 *      One arithmetic: f16 operands, fp32 accumulation on the f16 matrix pipe.  Argument errors of all entries, nothing
 *      launched, named with the entry and the item: a null pointer; K no multiple of 32 or beyond Y2_WIDE_HEAD_MAX_K;
 *      Cout outside 1..Y2_WIDE_HEAD_MAX_COUT; a pointer the kernels read in 16-byte units that is not 16-byte aligned. */
#define Y2_WIDE_HEAD_MAX_K 4096
#define Y2_WIDE_HEAD_MAX_COUT (65536 * 16)
/* host only: the bytes of the packed f16 operand image of a K -> Cout layer (Cout rounded up to the 256-column tile, K to
 * the 64-element K step); 0 where K or Cout break the rules above */
size_t y2_wide_head_packed_bytes(int K, int Cout);
/* W: fp32 filters [1][1][K][Cout] (the layout of a 1x1 layer's W) -> `packed`, 16-byte aligned, packed_bytes of it at
 * least y2_wide_head_packed_bytes: every byte of the image is written, the padding as zero.  One launch, no allocation.
 * Y2_ERR_ARG also: packed_bytes too small. */
int y2_wide_head_pack(const float* W, int K, int Cout, void* packed, size_t packed_bytes, void* stream);
/* out[m][c] = bias[c] + sum_k f16(x[m][k]) f16(W[k][c]): x fp32 [M][K], 16-byte aligned (what y2_forward writes), converted
 * inside the kernel; out fp32 [M][Cout], row stride Cout exactly, dword stores, nothing written past out + M * Cout.  One
 * launch, the same bits every run.  Y2_ERR_ARG also: M < 1; more than 2^31 - 1 tiles of 256 x 256. */
int y2_wide_head_forward(const float* x, const void* packed, const float* bias, int M, int K, int Cout, float* out,
                         void* stream);

/* ---- Training the wide head (csrc/wide_head_train.hip): the two backward products, the bias gradient and Darknet's SGD on
 *      the layer.  s = grad_scale > 0 is the loss scale of the half-precision modes; every result is an UNSCALED gradient,
 *      the contract of y2_backward_input.  The argument rules above hold; also Y2_ERR_ARG: M < 1; a grad_scale that is not
 *      finite and above 0; split < 0; a workspace that is null, too small or not 16-byte aligned where one is needed.  No
 *      allocation, one stream, no float atomics: partial sums are added in a fixed order, the same bits every run. */
/* host only, no GPU work: the number of workgroups that share the reduction of each product on a device of `cus` compute
 * units -- dx's over Cout in steps of 64 (128 x 128 tiles of [M][K]), dW's over M in steps of 64 (128 x 128 tiles of
 * [K][Cout]): ceil(cus / tiles), at most 64 and at most the steps, then evened out so that every split holds a step. */
int y2_wide_head_train_plan(int M, int K, int Cout, int cus, int* dx_split, int* dw_split);
/* the second operand image: f16 [K rounded up to 128][Cout rounded up to 64], Cout contiguous, padding zero -- what the data
 * gradient reads (the forward image has K contiguous).  _bytes: host only, 0 where K or Cout break the rules; pack2: one
 * launch, every byte written.  y2_wide_head_sgd_step keeps it current. */
size_t y2_wide_head_packed2_bytes(int K, int Cout);
int y2_wide_head_pack2(const float* W, int K, int Cout, void* packed2, size_t packed2_bytes, void* stream);
/* host only: the workspace of the entry below it.  split: 0 -- the plan's count for the current device; n >= 1 -- that many
 * (tests and measurements), evened out as the plan's.  One split needs no workspace: 0. */
size_t y2_wide_head_backward_input_workspace_bytes(int M, int K, int Cout, int split);
size_t y2_wide_head_backward_filter_workspace_bytes(int M, int K, int Cout, int split);
/* dx[m][k] = (1/s) sum_c f16(s dy[m][c]) f16(W[k][c]), fp32 accumulation.  dy fp32 [M][Cout], row stride Cout exactly, 4-byte
 * aligned (the tree loss's output): dword reads under a mask, nothing read past dy + M * Cout.  dx fp32 [M][K], every element
 * written, nothing behind it.  With more than one split: raw partials [split][M][K] in the workspace, then a finish pass. */
int y2_wide_head_backward_input(const float* dy, const void* packed2, int M, int K, int Cout, float grad_scale, float* dx,
                                void* workspace, size_t workspace_bytes, int split, void* stream);
/* dW[k][c] = (1/s) sum_m f16(x[m][k]) f16(s dy[m][c]), fp32 [K][Cout] (the layout of W), and db[c] = sum_m dy[m][c] in fp32
 * from the unconverted dy (a launch of its own).  x fp32 [M][K], 16-byte aligned.  Rows behind M contribute zero. */
int y2_wide_head_backward_filter(const float* x, const float* dy, int M, int K, int Cout, float grad_scale, float* dW, float* db,
                                 void* workspace, size_t workspace_bytes, int split, void* stream);
/* Darknet's SGD (y2_sgd_step's update; utils/solver.py sgd_step) on W [K][Cout] with weight decay and on b [Cout] without,
 * gradients times grad_mult, accum = K * Cout + Cout slots (W's, then b's) -- and both operand images rewritten from the new
 * W in the same launch, padding zero.  ctrl NULL: `lr` is the rate.  ctrl: the control block as it stands (the "next" member
 * of a joint step: found_inf set -- nothing moves; else ctrl.lr_t applies); this entry never advances it. */
int y2_wide_head_sgd_step(float* W, float* b, float* accum, const float* dW, const float* db, int K, int Cout, void* packed,
                          size_t packed_bytes, void* packed2, size_t packed2_bytes, const void* ctrl, float lr, float momentum,
                          float decay, float grad_mult, void* stream);

/* ---- ResNet-50 backbone swap (src/yolo2_nets/tf_resnet.py:12-32, src/pascal/pascal_train_resnet.py:37-50):
 *      graph-level operators on fp32 NHWC tensors that the conv-BN-leaky stacks do not have.  The 1x1 / 3x3
 *      convolutions of the bottleneck units (slim_dir/nets/resnet_v1.py:68-112) go through y2_conv2d /
 *      y2_conv2d_backward; a stride-2 unit = the stride-1 convolution + y2_subsample, slim's own definition of
 *      conv2d_same (slim_dir/nets/resnet_utils.py:77-122). --------------------------------------------------- */
/* slim.batch_norm (resnet_arg_scope: decay 0.997, epsilon 1e-5, scale; resnet_utils.py:230-257) on [rows][channels],
 * + optional residual add (before the activation) + optional ReLU: y = act(gamma (x - mean) / sqrt(var + eps) + beta
 * + residual).  is_training: batch statistics (saved in save_mean / save_var for the backward pass), moving
 * statistics updated when update_moving; else the moving statistics normalise. */
int y2_batch_norm_forward(const float* x, const float* residual, float* y, size_t rows, int channels, const float* gamma,
                          const float* beta, float* moving_mean, float* moving_var, float* save_mean, float* save_var,
                          float eps, float decay, int is_training, int update_moving, int relu, void* stream);
/* dx, dgamma, dbeta (and dresidual = the gradient entering before the activation, nullable) */
int y2_batch_norm_backward(const float* dy, const float* y, const float* x, float* dx, float* dresidual, size_t rows,
                           int channels, const float* gamma, const float* save_mean, const float* save_var, float eps,
                           int is_training, int relu, float* dgamma, float* dbeta, void* stream);
/* resnet_utils.subsample = max_pool2d([1,1], stride=factor) (resnet_utils.py:60-75): forward x [N,H,W,C] ->
 * y [N,ceil(H/f),ceil(W/f),C]; forward = 0: x is the gradient at the coarse grid, y the gradient at [N,H,W,C] */
int y2_subsample(const float* x, float* y, int N, int H, int W, int C, int factor, int forward, void* stream);
/* slim.max_pool2d(net, [3,3], stride=2) with padding 'SAME' (resnet_v1.py:198) and its gradient */
int y2_maxpool3x3s2(const float* x, float* y, int N, int H, int W, int C, void* stream);
int y2_maxpool3x3s2_backward(const float* x, const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* root block: conv2d_same(net, 64, 7, stride=2) on the image [N,H,W,3], filter HWIO [7][7][3][Cout] (resnet_v1.py:197) */
int y2_conv7x7s2(const float* x, const float* w, float* y, int N, int H, int W, int Cout, void* stream);
/* the same with the arithmetic type of the model (round 5): Y2_F16 / Y2_BF16 run it on the matrix pipe (operands rounded to
 * the type, fp32 accumulation and output; Cout <= 64, a multiple of 4), any other dtype is y2_conv7x7s2 */
int y2_conv7x7s2_t(const float* x, const float* w, float* y, int N, int H, int W, int Cout, int dtype, void* stream);
int y2_conv7x7s2_backward_filter_t(const float* x, const float* dy, float* dw, int N, int H, int W, int Cout, int dtype,
                                   void* stream);
int y2_conv7x7s2_backward_filter(const float* x, const float* dy, float* dw, int N, int H, int W, int Cout, void* stream);
/* slim.fully_connected (pascal_train_resnet.py:41-46; the flattened 7x7x2048 features -> 4096 -> S*S*(5B+C)) for a
 * batch of 1..128 rows: y [rows][out] = act(x [rows][in] * w [in][out] + bias), bias may be NULL, in_features a multiple
 * of 16.  One pass over the fp32 weights, converted in registers to `dtype` (0 fp32, 1 f16, 2 bf16) for the matrix
 * cores, fp32 accumulation and fp32 results.  Backward: dx [rows][in] = dy * w^T (NULL: skipped),
 * dw [in][out] = x^T * dy (NULL: skipped); dy is the gradient at the pre-activation (y2_bias_relu_backward). */
int y2_fully_connected(const float* x, const float* w, const float* bias, float* y, int rows, int in_features,
                       int out_features, int relu, int dtype, void* stream);
int y2_fully_connected_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, int rows,
                                int in_features, int out_features, int dtype, void* stream);
/* Round 5: the weight gradient of a fully connected layer fused with the guarded Adam update of that weight -- dW is
 * never stored (tf.train.AdamOptimizer(0.0005).minimize over yolo_fc1, src/pascal/pascal_train_resnet.py:41-50: 1.64 GB of
 * weights; writing, scanning and re-reading its gradient were 3 of the 10 passes over that size per step).  x [rows,in],
 * dz [rows,out] (gradient at the pre-activation, times the loss scale), w / m / v [in,out]; ctrl: the control block of
 * y2_adam_step_guarded AFTER that call advanced it for this step (found_inf: nothing moves; lr_t applies).  The caller's
 * overflow scan covers every OTHER gradient (the bias gradient of the same layer is the column sum of dz: a non-finite
 * dz is seen there; round 6: y2_range_check on x and dz makes the guard of THIS product explicit).  rows <= 256 in the 16-bit
 * types (128 in fp32): the batch -- or, data parallel, the batches of all replicas gathered: every rank then applies the
 * identical update from the identical operands instead of all-reducing a 1.64 GB gradient (yolo2_nets/tf_resnet.py). */
int y2_fc_adam_apply_guarded(const float* x, const float* dz, float* w, float* m, float* v, int rows, int in_features,
                             int out_features, int dtype, const void* ctrl, float beta1, float beta2, float eps,
                             float grad_mult, void* stream);
/* slim.fully_connected tail (pascal_train_resnet.py:41-46): y <- act(y + bias) in place; backward dz = dy [y > 0],
 * dbias = column sums; tf.nn.dropout(x, keep_prob) with a mask that is a function of (seed, index) */
int y2_bias_relu(float* y, const float* bias, size_t rows, int channels, int relu, void* stream);
int y2_bias_relu_backward(const float* dy, const float* y, float* dz, float* dbias, size_t rows, int channels, int relu,
                          void* stream);
int y2_dropout(const float* x, float* y, size_t n, float keep_prob, uint64_t seed, void* stream);
/* the same with the seed read from device memory at run time: a train step captured in a HIP graph replays with a new
 * mask every time (the host increments *seed between replays, or a captured kernel does) */
int y2_dropout_dev(const float* x, float* y, size_t n, float keep_prob, const uint64_t* seed, void* stream);

/* ---- optimizers on flat buffers (pascal_train_darknet.py:51, imagenet_train_darknet.py:58) */
int y2_adam_step(float* params, float* m, float* v, const float* grads, size_t n, int step, float lr,
                 float beta1, float beta2, float eps, float grad_mult, void* stream);
int y2_momentum_step(float* params, float* accum, const float* grads, size_t n, float lr, float momentum,
                     float grad_mult, void* stream);
/* The same updates guarded against half-precision gradient overflow (dynamic loss scaling; the fp32
 * reference cannot overflow): ctrl = 8 zero-initialised 32-bit device words {found_inf, step, skipped, -,
 * lr_t, ...}.  A scan sets ctrl.found_inf: y2_grad_check reads the context's SENTINEL ranges of its bound gradient
 * buffer (b / gamma / beta of every layer and one row of the first filter, ~30 k floats: every non-finite value of the
 * backward pass reaches them -- an inf / NaN in a layer's incoming gradient makes the channel sums dbeta
 * non-finite, a dy that overflows at its own f16 store is an operand of the dgrad below it, and the first layer's
 * dy feeds its filter gradient directly); y2_grad_check_full reads every element of any buffer.
 * The guarded step then skips as a whole when found_inf is set (params, slots and the device-side step
 * counter untouched, ctrl.skipped += 1); otherwise ctrl.step advances and Adam's lr_t is computed on the
 * device for it.  No host synchronisation. */
int y2_grad_check(y2_ctx* ctx, void* ctrl, void* stream);
/* the same scan OR-ed into ctrl.found_inf WITHOUT clearing it first: further stacks of ONE composed graph scanned into
 * the control block the first stack's y2_grad_check cleared -- the step is then all-or-nothing over the whole graph */
int y2_grad_check_more(y2_ctx* ctx, void* ctrl, void* stream);
int y2_grad_check_full(const float* grads, size_t n, void* ctrl, void* stream);
/* Round 6.  ctrl.found_inf |= any x[i] that is non-finite or beyond +-limit; the flag is NOT cleared first (call it between
 * y2_grad_check_full and the guarded update).  For operands that a fused update rounds to a narrower type without ever
 * storing the gradient: y2_fc_adam_apply_guarded rounds dz to f16 / bf16 inside the kernel, so a |dz| above 65504 is finite in
 * every stored fp32 gradient it feeds and inf in the weight's (src/pascal/pascal_train_resnet.py:41-50, yolo_fc1). */
int y2_range_check(const float* x, size_t n, float limit, void* ctrl, void* stream);
int y2_adam_step_guarded(float* params, float* m, float* v, const float* grads, size_t n, void* ctrl, float lr,
                         float beta1, float beta2, float eps, float grad_mult, void* stream);
int y2_momentum_step_guarded(float* params, float* accum, const float* grads, size_t n, void* ctrl, float lr,
                             float momentum, float grad_mult, void* stream);

/* The optimizer step of a context's bound parameters / gradients FUSED with the re-pack of its filters into the
 * MFMA operand layouts (the update reads and writes every filter anyway; y2_forward then finds the packed copies
 * current and skips its own re-pack pass).  Same arithmetic as y2_adam_step / y2_momentum_step.  ctrl: NULL for
 * the plain step number `step`, or the guard words of the *_guarded forms (run y2_grad_check first).  Other
 * contexts bound to the same parameter buffer must still call y2_params_changed. */
/* (ctrl with step < 0: do not advance the control block -- a further stack of a composed graph whose first stack's call
 * advanced it already: ONE step counter and lr_t for the whole graph) */
int y2_adam_step_packed(y2_ctx* ctx, float* m, float* v, void* ctrl, int step, float lr, float beta1, float beta2,
                        float eps, float grad_mult, void* stream);
int y2_momentum_step_packed(y2_ctx* ctx, float* accum, void* ctrl, float lr, float momentum, float grad_mult,
                            void* stream);

/* ---- Darknet's SGD solver (YOLOv2's recipe; the reference has no counterpart.  Specification: utils/solver.py).
 * The record: Darknet's learning_rate, momentum, decay, policy, burn_in, power, steps / scales and max_batches.
 *   rate(t), t >= 1 the applied step:  t < burn_in: lr (t / burn_in)^power;  else constant: lr;  steps: lr times
 *   scales[i] of every steps[i] <= t;  poly: lr max(0, 1 - t / max_batches)^power.  Double arithmetic on the widened
 *   floats, powers as repeated products, one cast to float: the host routine and the device schedule agree bit for bit.
 *   update:  gd = g grad_mult (+ decay p for convolution filters only);  accum = momentum accum + gd;  p -= rate accum.
 * The losses of this library are batch means: learning_rate times the mean gradient is Darknet's learning_rate / batch
 * times its summed gradient, so the cfg's value is the one to give. */
#define Y2_POLICY_CONSTANT 0
#define Y2_POLICY_STEPS 1
#define Y2_POLICY_POLY 2
#define Y2_SOLVER_MAX_STEPS 8
typedef struct y2_sgd_solver {
    float learning_rate, momentum, decay;
    int policy, burn_in, power, max_batches, nsteps;
    int steps[Y2_SOLVER_MAX_STEPS];
    float scales[Y2_SOLVER_MAX_STEPS];
} y2_sgd_solver;
/* host only, no GPU work: *rate = rate(t).  Y2_ERR_ARG on an invalid record or t < 1 */
int y2_solver_rate(const y2_sgd_solver* solver, int t, float* rate);
/* The step over a bound training context's parameters / gradients: y2_sgd_step is the flat form (the packed filter
 * copies are marked stale, as by y2_params_changed), y2_sgd_step_packed the one fused with the filter re-pack, same
 * bits.  accum: one slot per parameter.  ctrl / step as y2_adam_step_packed: ctrl NULL -- the host gives step >= 1
 * and computes the rate; ctrl with step >= 0 -- run y2_grad_check first; a clean flag advances ctrl.step and sets
 * ctrl.lr_t = rate(ctrl.step) on the device, a set flag counts ctrl.skipped and moves nothing, the schedule included;
 * ctrl with step < 0 -- another stack of the same composed step advanced the control block: use it as it stands. */
int y2_sgd_step(y2_ctx* ctx, float* accum, void* ctrl, int step, const y2_sgd_solver* solver, float grad_mult,
                void* stream);
int y2_sgd_step_packed(y2_ctx* ctx, float* accum, void* ctrl, int step, const y2_sgd_solver* solver, float grad_mult,
                       void* stream);

/* The reference's train_op as ONE call (optimizer.minimize(loss) = compute_gradients + apply_gradients,
 * src/pascal/pascal_train_darknet.py:49-51; imagenet_train_darknet.py:58): y2_backward over all layers, then, with
 * ctrl, the sentinel overflow check (y2_grad_check), then y2_adam_step_packed / y2_momentum_step_packed -- and the
 * same results, bit for bit.  What changes is the schedule on the single-GPU path: for the pooled 3-channel first
 * layer every layer above it is checked and updated on the weight-gradient stream while the first layer's
 * gradient kernel runs (their gradients are final by then; the first layer's overflow sentinel is replaced by a
 * non-finite marker on the gradient tensor that feeds it, which decides the step before that kernel ends).
 * Data-parallel callers, whose all-reduce sits between the two halves, keep the separate calls. */
int y2_backward_adam(y2_ctx* ctx, const float* dout, float* m, float* v, void* ctrl, int step, float lr, float beta1,
                     float beta2, float eps, float grad_mult, void* stream);
int y2_backward_momentum(y2_ctx* ctx, const float* dout, float* accum, void* ctrl, float lr, float momentum,
                         float grad_mult, void* stream);

/* ---- single-op entry points (tf.nn.conv2d 'SAME' stride 1, darknet.py:20-21) used by the
 *      per-op parity tests; channel counts are padded internally to the kernels' granularity */
size_t y2_conv2d_workspace_bytes(int N, int H, int W, int Cin, int Cout, int k, int dtype);
int y2_conv2d(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin,
              int Cout, int k, int dtype, void* workspace, void* stream);
int y2_conv2d_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, int N, int H,
                       int W, int Cin, int Cout, int k, int dtype, void* workspace, void* stream);

/* ---- launch log: which kernel form every forward / dgrad convolution and every weight gradient took.  Host memory
 *      only (it never touches the GPU), process-wide, off by default; while off a launch pays one branch.  A record is
 *      Y2_LAUNCH_LOG_INTS ints -- exactly what selects a kernel instantiation or a distinct code path inside one:
 *        convolution     {0, launch dtype, is_dgrad, kernel kind, tile / config, K split (0/1),
 *                         epilogue: 0 plain, 1 batch-norm statistics, 2 fused batch-norm-backward reduce}
 *        weight gradient {1, launch dtype, kernel kind, tile, split-K (0/1), route of the partial sums, 0}
 *      (kinds, tiles and routes: the enums of csrc/kernels.h).  The folded-inference epilogue is not part of the key.
 *      y2_launch_log_enable(1) clears the log and starts recording, (0) stops (the records stay readable);
 *      y2_launch_log_read copies min(logged, max_records) records to the host array `out` (may be NULL with 0) and
 *      returns the number logged. */
#define Y2_LAUNCH_LOG_INTS 7
int y2_launch_log_enable(int enable);
int y2_launch_log_read(int* out, int max_records);

/* ---- MXFP8 quantiser (the Y2_FP8 number format above): fp32 x [rows][C], C % 32 == 0 -> e4m3fn elements q [rows][C]
 *      + E8M0 scales [rows][C / 32] (one per 32 consecutive values of a row), device buffers */
int y2_mx_quantize(const float* x, size_t rows, int C, uint8_t* q, uint8_t* scales, void* stream);

/* ---- device-resident input batches (img_dataset/device_voc.py): the reference's imdb.get() (src/img_dataset/
 *      pascal_voc.py:42-86: cv2.resize to image_size, optional mirror, label grid) from ONE copy of the decoded images
 *      kept at native resolution in device memory, for any output size.  Both calls are bit-equal to the host code of
 *      img_dataset/pascal_voc.py (resize_bilinear_u8, encode_boxes, flip_label, the float32 cast of get_u8).
 *      `table`: int64 [entries][5] = {byte offset of the image in `pool`, height, width, row pitch in bytes, flip};
 *      pixels are uint8 BGR, 3 bytes per pixel, rows `pitch` bytes apart.  Offsets and pitches that are multiples of
 *      16 (and pitch <= 4096) let the kernel stage rows with 16-byte loads; anything else is read in place, same
 *      result.  `index`: int32 [n], the table entry of each batch slot (NULL: slot i is entry i).  All pointers are
 *      device memory. */
#define Y2_RESIZE_MAX_OUT_W 1024 /* columns of the kernel's coefficient table: out_w beyond it is an argument error */
/* out [n][out_h][out_w][3] uint8: cv2.resize(img, (out_w, out_h)) INTER_LINEAR on uint8 (half-pixel centres, no
 * antialias, 11-bit weights from float64 coefficients, (top * wy0 + bot * wy1 + 2^21) >> 22), then [:, ::-1, :] where
 * the entry's flip is set. */
int y2_resize_bilinear_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int out_h,
                                int out_w, uint8_t* out, void* stream);
/* The letterboxed input of the anchor detector (img_dataset/pascal_voc.letterbox_u8 and letterbox_geometry are the
 * specification, bit for bit).  Geometry, integers only, as Darknet's letterbox_image: for an image of im_w x im_h and a
 * square of `size`, if im_h <= im_w then new_w = size, new_h = max(1, im_h * size / im_w), else new_h = size,
 * new_w = max(1, im_w * size / im_h) (C division, 64-bit products); ox = (size - new_w) / 2, oy = (size - new_h) / 2 are
 * the left / top bars, and the right / bottom bar gets the odd pixel.  Host only, no GPU work:
 * geometry[4] = new_w, new_h, ox, oy.  Y2_ERR_ARG on a null pointer or a value below 1. */
int y2_letterbox_geometry(int im_h, int im_w, int size, int* geometry);
/* out [n][size][size][3] uint8, pool / table / index as y2_resize_bilinear_u8_batch: a canvas of `fill` (0..255) whose
 * rows oy .. oy + new_h - 1 and columns ox .. ox + new_w - 1 hold the image resized to new_w x new_h exactly as
 * y2_resize_bilinear_u8_batch resizes it to that size.  A letterbox in DESTINATION space: the picture's edge is not
 * blended with the fill.  The flip column of the table is not read; an empty table row gives a canvas of fill alone.
 * `size` a multiple of 4 up to Y2_RESIZE_MAX_OUT_W and `out` 4-byte aligned (the bars are written with vector stores),
 * else an argument error.  One launch. */
int y2_letterbox_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int size, int fill,
                          uint8_t* out, void* stream);
/* labels [n][S][S][5 + num_class] float32 (zero-filled here): `boxes` double [entries][max_obj][5] = xmin, ymin, xmax,
 * ymax, class index in 1-based pixels of the original image, in annotation order; `counts` int32 [entries].  Ratios
 * image_size / width, clamp to [0, image_size - 1], centre / size, cell int(c * S / image_size), the first object of a
 * cell wins; a flipped entry mirrors the columns and stores image_size - 1 - x. */
int y2_encode_labels(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index, int n,
                     int max_obj, int image_size, int S, int num_class, float* labels, void* stream);

/* ---- training augmentation on the same pool (img_dataset/augment.py is the specification; both calls are bit-equal to
 *      it): `params` double [n][8] in device memory, one row per BATCH SLOT = {x0, y0, cw, ch, flip, hue, sat, exp}.
 *      x0, y0, cw, ch: a window of the source in integer pixels (columns x0 .. x0 + cw - 1), which may extend beyond
 *      the image on any side; flip: mirror on top of the entry's (the two cancel); hue, sat, exp: float32 values of
 *      the colour distortion, (0, 1, 1) = none.  The row {0, 0, width, height, 0, 0, 1, 1} reproduces the two calls
 *      above.  x0, y0, cw, ch are integers; a fraction is cut off (toward zero) by both calls.  A row without a window (cw < 1 or ch < 1, or not a number) gives an image of `fill` alone and an empty
 *      grid.  `pool`, `table`, `index`, `boxes`, `counts` as above. */
/* out [n][out_h][out_w][3] uint8: the window (pixels outside the image = `fill`, 0..255) resized as above with cw x ch
 * for the source size, mirrored, then through HSV in float32: hue + 6 * hue wrapped into [0, 6), min(s * sat, 1),
 * min(v * exp, 1), (int)(x * 255 + 0.5) (augment.distort_hsv_u8).  One launch; out_w <= Y2_RESIZE_MAX_OUT_W. */
int y2_augment_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, const double* params, int n,
                        int out_h, int out_w, int fill, uint8_t* out, void* stream);
/* y2_encode_labels with the boxes following the window: x = (bx - 1 - x0) * (image_size / cw), y likewise; an object
 * whose unclamped centre lies outside [0, image_size) is dropped (augment.encode_boxes_window). */
int y2_encode_labels_window(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                            const double* params, int n, int max_obj, int image_size, int S, int num_class,
                            float* labels, void* stream);
/* The label of the anchor model that keeps EVERY object (augment.encode_box_list, bit-equal): truth float32
 * [n][max_boxes][5] = cx, cy, w, h in pixels of the resized input and the class index, ntruth int32 [n].  Per object the
 * arithmetic of y2_encode_labels_window without the "cell already taken" rule; objects in annotation order, those beyond
 * max_boxes dropped in that order, rows at and beyond ntruth zero.  `params` NULL: the identity row of every entry (the
 * plain path of y2_encode_labels).  A row without a window gives an empty list.  One 64-lane wave per image. */
#define Y2_MAX_BOXES 1024 /* rows of a box list; more is an argument error */
int y2_encode_box_list(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                       const double* params, int n, int max_obj, int image_size, int max_boxes, float* truth,
                       int32_t* ntruth, void* stream);
/* y2_encode_box_list with Darknet's shuffle-then-cut (augment.encode_box_list_draw, bit-equal).  `keys` uint32 [n] in
 * device memory, one per batch slot.  An image whose window keeps at most max_boxes objects gives y2_encode_box_list's
 * rows, whatever its key.  One that keeps more gives exactly max_boxes rows: the objects with the smallest
 * (augment.box_rank(key, j), j), j the annotation index, written in annotation order.  `keys` NULL: y2_encode_box_list's
 * result.  max_obj beyond Y2_DRAW_MAX_OBJ (the kernel keeps one ballot bit per object in LDS) is an argument error.  One
 * 64-lane wave per image, no atomics. */
#define Y2_DRAW_MAX_OBJ 1024
int y2_encode_box_list_draw(const double* boxes, const int32_t* counts, const int64_t* table, const int32_t* index,
                            const double* params, const uint32_t* keys, int n, int max_obj, int image_size,
                            int max_boxes, float* truth, int32_t* ntruth, void* stream);

/* ---- the classifier's augmentation on the same pool (img_dataset/augment_cls.py is the specification, bit for bit):
 *      mirror, rotation, scale and crop as ONE affine map.  `params` double [n][9] in device memory, one row per batch
 *      slot = {m00, m01, m02, m10, m11, m12, hue, sat, exp}: output pixel (u, v) reads the source coordinate
 *      sx = (m00 * u + m01 * v) + m02, sy = (m10 * u + m11 * v) + m12 (float64, every operation rounded on its own).  A
 *      coordinate that is not finite or of magnitude >= 2^30 gives `fill`; else x0 = floor(sx), weight
 *      (int)((sx - x0) * 2048 + 0.5), four taps that read `fill` (0..255) outside the image, the int32 blend of the
 *      calls above, then the colour stage of y2_augment_u8_batch ((0, 1, 1) = none; fill pixels pass through it too).
 *      `params` NULL: every slot takes the plain stretch of its entry (augment_cls.identity_row of the table row, formed
 *      in the kernel) and no colour stage.  `labels` int32 [entries] with `labels_out` int32 [n]: labels_out[b] =
 *      labels[index[b]] in the same launch; both NULL: no labels.  The flip column of the table is not read; an empty
 *      table row writes no pixel.  Y2_ERR_ARG: n outside 1..65535, out_h < 1, out_w not a positive multiple of 4, fill
 *      outside 0..255, `out` not 4-byte aligned, exactly one of labels / labels_out NULL.  One launch. */
int y2_warp_u8_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, const double* params,
                     const int32_t* labels, int n, int out_h, int out_w, int fill, uint8_t* out, int32_t* labels_out,
                     void* stream);

/* ---- evaluation of the grid detector from the same pool (pascal/pascal_eval_darknet.py; utils/detect_batch.py is the
 *      specification and both calls are bit-equal to it): per image, the head's output -> boxes in the pixels of the
 *      ORIGINAL image after a score-ordered class-aware NMS, then the VOC devkit's matching against the image's ground
 *      truth.  Not in the reference (it has no evaluation code).  Only the precision / recall curve, one sort across all
 *      images, stays on the host (detect_batch.map_from_flags).  `table`, `index`, `boxes`, `counts` as above; each image
 *      takes its height and width from its table row, and the flip column is not read (evaluation uses unmirrored
 *      entries).  All pointers are device memory. */
#define Y2_DETECT_MAX_CANDIDATES 1024 /* S * S * B of one image (608 x 608 with B = 2: 722); more is an argument error */
#define Y2_MATCH_MAX_OBJECTS 1024     /* max_obj of the box table; more is an argument error */
/* predict [n][S][S][num_class + 5 B] fp32.  Candidate i = cell * B + b (cell = row * S + column): the float64 products
 * x, y, w, h of y2_decode_detections, upper left corner x - floor(w / 2), y - floor(h / 2), the inclusive box
 * (ulx, uly, ulx + w - 1, uly + h - 1) cut to [0, width - 1] x [0, height - 1], then + 1 (the annotation's pixels are
 * 1-based); class = first maximum of the class values; score = the confidence.  Valid: confidence > object_thresh (not
 * NaN), the four products finite and below 2^30 in magnitude (checked before any conversion to int), and the cut box not
 * empty.  The valid candidates are walked in descending score (ties: ascending i); a kept box suppresses every later box
 * of the SAME class whose IoU with it (float64, + 1 extents) is > iou_thresh; at most max_out are kept.
 * det int32 [n][max_out][6] = xmin, ymin, xmax, ymax, class, i (unused rows all -1); score [n][max_out] (unused 0);
 * count int32 [n].  One workgroup per image. */
int y2_detect_grid_batch(const float* predict, const int64_t* table, const int32_t* index, int n, int S, int B,
                         int num_class, float object_thresh, float iou_thresh, int max_out, int* det, float* score,
                         int* count, void* stream);
/* The same for the YOLOv2 anchor head, from its RAW output (pascal/pascal_eval_yolov2.py; specification:
 * utils/detect_batch.anchor_detect on the outputs of y2_decode_anchors + y2_class_argmax, bit for bit).
 * net [n][S][S][B][5 + num_class] fp32 (tx, ty, tw, th, to, class logits), anchors [B][2] in cell units (device memory).
 * Candidate i = cell * B + b: cx, cy, w, h relative to the image and score[c] = sigmoid(to) * softmax(logits)[c] exactly
 * as y2_decode_anchors forms them in float32; class = first maximum of score[c], score = that maximum.  The float64
 * products cx * width, cy * height, w * width, h * height (the resize is a plain stretch) then go the way of
 * y2_detect_grid_batch: validity (score > score_thresh), truncation, corner, cut, + 1, ordering, class-aware walk, and the
 * same det / score / count conventions.  S * S * B up to Y2_DETECT_ANCHOR_MAX_CANDIDATES, B up to 16.  One workgroup per
 * image, one launch. */
#define Y2_DETECT_ANCHOR_MAX_CANDIDATES 2048 /* 608 x 608 with B = 5: 1805; more is an argument error */
int y2_detect_anchor_batch(const float* net, const float* anchors, const int64_t* table, const int32_t* index, int n,
                           int S, int B, int num_class, float score_thresh, float iou_thresh, int max_out, int* det,
                           float* score, int* count, void* stream);
/* y2_detect_anchor_batch for a batch made by y2_letterbox_u8_batch at net_size = 32 S (else an argument error): the
 * four float64 products are replaced by the exact inverse of that embedding, with new_w, new_h, ox, oy of
 * y2_letterbox_geometry(height, width, net_size) and in this operation order:
 *   sx = width / new_w, sy = height / new_h;  x = (cx * net_size - ox) * sx;  y = (cy * net_size - oy) * sy;
 *   w = (w * net_size) * sx;  h = (h * net_size) * sy
 * and everything after them is unchanged: a box in a bar maps outside the image and is cut, or empty and dropped, by the
 * existing rule (specification: utils/detect_batch.anchor_detect with net_size, bit for bit). */
int y2_detect_anchor_batch_lb(const float* net, const float* anchors, const int64_t* table, const int32_t* index, int n,
                              int S, int B, int num_class, float score_thresh, float iou_thresh, int max_out,
                              int net_size, int* det, float* score, int* count, void* stream);
/* One row per (candidate, class) instead of one per candidate, as Darknet's `valid` writes them (specification:
 * utils/detect_batch.anchor_detect_classes on the outputs of y2_decode_anchors, bit for bit).  Class c of an image is a
 * segment of its own: the rows of y2_detect_anchor_batch had every candidate the class c and the score score[c], so a
 * candidate is valid in every class whose score is > score_thresh, and the ordering and the walk run per class.
 * det int32 [n][num_class][max_per_class][6] = xmin, ymin, xmax, ymax, c, i (unused rows all -1);
 * score [n][num_class][max_per_class] (unused 0); count int32 [n][num_class].  The [n * num_class][max_per_class][6] view
 * of det, with count and an index vector that names each image num_class times, is what y2_voc_match_batch reads.
 * Limits as y2_detect_anchor_batch, and n up to 65535.  One workgroup per (class, image), one launch; nothing is
 * allocated. */
int y2_detect_anchor_classes_batch(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                   int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                   int max_per_class, int* det, float* score, int* count, void* stream);
/* y2_detect_anchor_classes_batch with the letterbox map of y2_detect_anchor_batch_lb (specification:
 * utils/detect_batch.anchor_detect_classes with net_size, bit for bit). */
int y2_detect_anchor_classes_batch_lb(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                      int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                      int max_per_class, int net_size, int* det, float* score, int* count,
                                      void* stream);
/* flags int32 [n][max_out]: 1 true positive, 0 false positive, 2 ignored, -1 beyond count.  The rows of an image are
 * walked in order (descending score): among the image's objects of the row's class, the first maximum of the float64
 * IoU, taken objects included; none, or IoU < iou_thresh: false positive; else a difficult object: ignored; an object
 * not yet taken: true positive, and it is taken; else false positive (utils/voc_eval.eval_class for one image).
 * `difficult`: uint8 [entries][max_obj].  `det` rows may come from any detector (columns 0..4 are read); `score` is not
 * read and may be NULL.  One 64-lane wave per image. */
int y2_voc_match_batch(const int* det, const float* score, const int* count, const double* boxes,
                       const int32_t* counts, const uint8_t* difficult, const int32_t* index, int n, int max_obj,
                       int max_out, float iou_thresh, int* flags, void* stream);

/* ---- Darknet's test-time protocol (csrc/darknet_io.hip): the input its `letterbox_image` makes and the rows
 *      its `valid` writes.  Everything is float32 in the stated operation order, double where it says so, no fused
 *      multiply-add; the specifications are img_dataset/pascal_voc.letterbox_darknet and utils/detect_batch
 *      (darknet_unmap, box_iou_darknet, anchor_detect_classes_darknet, match_image_f), bit for bit. */
/* out [n][size][size][3] float32, RGB in [0, 1], pool / table / index as y2_letterbox_u8_batch: a canvas of 0.5 whose
 * rectangle new_w x new_h at (ox, oy) of y2_letterbox_geometry holds Darknet's resize_image of the picture, with
 * src(x, y, k) = float(byte of channel 2 - k) / 255:
 *   horizontal, per source row: w_scale = float(w - 1) / float(new_w - 1); column c: sx = float(c) * w_scale, ix = (int)sx,
 *     dx = sx - float(ix), part = (1 - dx) * src(ix) + dx * src(ix + 1); the last column (and a source one pixel wide) is
 *     src(w - 1), copied;
 *   vertical: h_scale = float(h - 1) / float(new_h - 1); row r: sy = float(r) * h_scale, iy = (int)sy, dy = sy - float(iy),
 *     v = (1 - dy) * part(iy), then v = v + dy * part(iy + 1) unless r is the last row or h is 1.
 * The last row never receives the second term, as in Darknet: where float(new_h - 1) * h_scale rounds below h - 1 it is
 * nearly black.  An output extent of 1 takes the scale 0; ix, iy and their + 1 neighbours are clamped to the last column /
 * row (never with a non-zero weight), so no read leaves an image.  A letterbox in DESTINATION space; the flip column is not
 * read; an empty table row gives a canvas of 0.5.  Y2_ERR_ARG: a null pointer, n outside 1..65535, `size` not a multiple
 * of 32 in 32..Y2_RESIZE_MAX_OUT_W, `out` not 16-byte aligned.  One launch, from the uint8 pool to the network's input. */
int y2_letterbox_darknet_batch(const uint8_t* pool, const int64_t* table, const int32_t* index, int n, int size,
                               float* out, void* stream);
/* y2_detect_anchor_classes_batch_lb's arguments, grid, ordering (descending score, ties by ascending candidate) and cap, for
 * a batch made by y2_letterbox_darknet_batch at net_size = 32 S (else an argument error), with Darknet's boxes.  From
 * cx, cy, w, h of y2_decode_anchors, N = net_size and new_w, new_h of y2_letterbox_geometry:
 *   bx = float((double(cx) - double(N - new_w) / 2. / double(N)) / double(float(new_w) / float(N)));
 *   bw = w * (float(N) / float(new_w));  then bx = bx * float(width), bw = bw * float(width);  by, bh likewise.
 * Valid in class c: score[c] > score_thresh (not NaN) and the four values finite; nothing else.  A kept box suppresses every
 * later box of the class whose float32 IoU on (bx, by, bw, bh) is > iou_thresh: overlap = min(x1 + w1 / 2, x2 + w2 / 2) -
 * max(x1 - w1 / 2, x2 - w2 / 2) per axis, inter = 0 if either is negative else their product, union = (aw * ah + bw * bh) -
 * inter; a NaN suppresses nothing.  Row: xmin = float(double(bx) - double(bw) / 2. + 1.) raised to 1, xmax =
 * float(double(bx) + double(bw) / 2. + 1.) lowered to float(width), ymin / ymax likewise; a box empty after that is kept.
 * det int32 [n][num_class][max_per_class][6]: words 0..3 are the BIT PATTERNS of the float32 xmin, ymin, xmax, ymax, word 4
 * the class, word 5 the candidate (unused rows all -1); score and count as y2_detect_anchor_classes_batch. */
int y2_detect_anchor_classes_batch_dk(const float* net, const float* anchors, const int64_t* table, const int32_t* index,
                                      int n, int S, int B, int num_class, float score_thresh, float iou_thresh,
                                      int max_per_class, int net_size, int* det, float* score, int* count,
                                      void* stream);
/* y2_voc_match_batch with words 0..3 of a det row read as float32 (the rows of y2_detect_anchor_classes_batch_dk): the
 * float64 IoU with + 1 extents works on those four values promoted to double.  The same flags, limits and launch. */
int y2_voc_match_batch_f(const int* det, const float* score, const int* count, const double* boxes,
                         const int32_t* counts, const uint8_t* difficult, const int32_t* index, int n, int max_obj,
                         int max_out, float iou_thresh, int* flags, void* stream);

/* ---- Detection on a word-tree head from the tree's node (csrc/detect_tree.hip; DESIGN.md 9, "Detection from the node").
 *      net is the RAW head [n][S][S][B][5 + num_class] and top int32 [n * S * S * B] the node of every candidate
 *      (y2_word_tree_top): candidate i of an image has the box of y2_decode_anchors, the score sigmoid(to) and the class
 *      top[img * S * S * B + i].  A candidate whose top lies outside [0, num_class) -- the -1 of a row the walk skipped --
 *      is not valid; top is compared and stored, never used as an index.  Elements 0..4 of a head row are read and nothing
 *      behind them.  Limits, argument errors, det / score / count and their fill values as y2_detect_anchor_batch, plus a
 *      null top.  One workgroup per image, one launch. */
/* The integer rows of y2_detect_anchor_batch (net_size 0: the plain stretch) or y2_detect_anchor_batch_lb (net_size = 32 S;
 * anything else is an argument error): the float64 products, validity, cut, ordering and class-aware walk are theirs.  With
 * score_thresh >= 0 and top from y2_word_tree_top (obj_thresh < 0, or obj_thresh = score_thresh) the rows are bit for bit
 * those of that entry on the rows y2_word_tree_head wrote (specification: utils/detect_batch.anchor_detect(boxes, so,
 * top, ...)). */
int y2_detect_anchor_tree_batch(const float* net, const int* top, const float* anchors, const int64_t* table,
                                const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                                float iou_thresh, int max_out, int net_size, int* det, float* score, int* count,
                                void* stream);
/* The same under Darknet's protocol (net_size = 32 S required): the box, validity (score > score_thresh and four finite
 * values, nothing else), float centre-box IoU and row words of y2_detect_anchor_classes_batch_dk, but FLAT rows
 * [n][max_out][6] in one descending order per image (ties by ascending candidate) under the class-aware walk: a kept box
 * suppresses later boxes of the same node.  y2_voc_match_batch_f reads these rows as they are (specification:
 * utils/detect_batch.anchor_detect_tree_darknet). */
int y2_detect_anchor_tree_batch_dk(const float* net, const int* top, const float* anchors, const int64_t* table,
                                   const int32_t* index, int n, int S, int B, int num_class, float score_thresh,
                                   float iou_thresh, int max_out, int net_size, int* det, float* score, int* count,
                                   void* stream);

/* ---- COCO's bounding-box matching (csrc/coco.hip; DESIGN.md 9, "COCO evaluation"; specification:
 *      utils/coco_eval.match_segment, numpy float64, bit for bit -- a restatement of COCOeval.evaluateImg with
 *      iouType = "bbox", useCats = 1 and of the mask API's bbIou).  Not in the reference.
 * det [n][max_out][6], count [n], index [n] or NULL: as y2_voc_match_batch reads them (columns 0..4 of a row; with
 * per-class rows a segment is one (image, class) and index names each image num_class times).  boxes float64
 * [entries][max_obj][5] = x, y, w, h, class of every annotation in file order, in COCO's own convention (zero-based
 * continuous corner, no + 1 extent); area float64 [entries][max_obj], the annotation's `area` field; crowd uint8
 * [entries][max_obj]; counts int32 [entries].  thresholds float64 [T], area_ranges float64 [A][2] = lo, hi.  All pointers
 * are device memory.
 * A row's box: row_form 0, the integer rows of y2_detect_anchor_classes_batch[_lb] (1-based inclusive corners):
 * x = xmin - 1, y = ymin - 1, w = xmax - xmin + 1, h = ymax - ymin + 1; row_form 1, the float rows of
 * y2_detect_anchor_classes_batch_dk (both corners carry Darknet's + 1): x = double(xmin) - 1, y = double(ymin) - 1,
 * w = double(xmax) - double(xmin), h likewise.
 * IoU(d, g, crowd), every operation a separate double operation: da = dw * dh; ga = gw * gh; ow = min(dx + dw, gx + gw) -
 * max(dx, gx), 0 if ow <= 0; oh likewise; i = ow * oh; u = crowd ? da : (da + ga) - i; i / u.
 * For every area range a and threshold t on their own: an object is IGNORED if it is crowd or its area is < lo or > hi.
 * The rows are walked in order (descending score).  Per row best = min(thresholds[t], 1 - 1e-10), no match; first the
 * non-ignored objects of the row's class in annotation order: one already matched under (a, t) is skipped, one whose IoU
 * is < best is skipped, else best = IoU and it is the match (an equal IoU moves the match to the later object); only if
 * none was found, the ignored objects of the class by the same rules, except that a crowd object is never skipped for
 * being matched and its IoU is the crowd form.  A match becomes matched; the row's value is 1 (true positive) if the
 * match is not ignored, else 2 (ignored).  Without a match the value is 2 if the row's own w * h is < lo or > hi, else 0
 * (false positive).
 * match int32 [n][max_out][A]: bits 2t, 2t + 1 of word a hold the value under (a, t), the other bits 0; rows at or beyond
 * count are all -1.  Non-finite rows are not specified.  Y2_ERR_ARG, nothing launched: a null pointer (index may be
 * NULL), n outside 1..Y2_COCO_MAX_SEGMENTS, max_obj outside 1..Y2_COCO_MAX_OBJECTS, max_out outside 1..Y2_COCO_MAX_ROWS,
 * T outside 1..Y2_COCO_MAX_THRESHOLDS, A outside 1..Y2_COCO_MAX_AREAS, T * A > 64, row_form not 0 or 1.
 * One 64-lane wave per segment, lane = (a, t); one launch, nothing allocated, no synchronisation, no atomics. */
#define Y2_COCO_MAX_SEGMENTS (65535 * 80) /* n: 65535 images of 80 classes */
#define Y2_COCO_MAX_OBJECTS 256           /* max_obj: 116 bytes of LDS per object (29 KB here, and several waves per CU
                                             at COCO's real maximum of about a hundred annotations per image) */
#define Y2_COCO_MAX_ROWS 65536            /* max_out (COCO's maxDets is 100) */
#define Y2_COCO_MAX_THRESHOLDS 16         /* T: two bits per threshold in one int32 word */
#define Y2_COCO_MAX_AREAS 4               /* A */
int y2_coco_match_batch(const int* det, const int* count, const double* boxes, const double* area,
                        const uint8_t* crowd, const int32_t* counts, const int32_t* index, int n, int max_obj,
                        int max_out, const double* thresholds, int T, const double* area_ranges, int A, int row_form,
                        int* match, void* stream);

/* ---- classifier scoring over several views of an image (csrc/score.hip; specification: utils/score_views.py, float64).
 * logits [n * views][classes] fp32, row b * views + v is view v of image b.  Per view p_v[c] = exp(x_v[c] - max_v) /
 * sum_c exp(x_v[c] - max_v), then p[c] = (1 / views) * sum_v p_v[c] (Darknet's validate_classifier_10 averages the
 * predictions of the views).  The classes are ordered larger score first, equal scores by the lower class index; the
 * score is the LOGIT for views == 1 (the order of tf.nn.top_k / tf.argmax: two logits that round to one probability still
 * rank as the logits do) and the float32 p[c] for views > 1.
 *   prob    [n][classes] or NULL: p
 *   top_idx, top_val [n][k]: the j-th class in that order and its p; for j >= classes index -1, value 0
 *   rank    [n] or NULL: the number of classes ordered before labels[b], 0-based
 *   hits    [4] or NULL, ACCUMULATED (zero it before the first batch): images, top-1 (rank == 0), top-k (rank < k), labels
 *           outside 0 .. classes - 1.  Only slots b < n_valid count (the repeated last entry of a short final batch);
 *           every slot gets its other outputs.
 * A label outside 0 .. classes - 1 forms no address: rank = classes, a miss, one more in hits[3].  views 1..16, k 1..8,
 * n_valid 0..n; rank and hits need labels.  One workgroup per image, one launch; reductions in a fixed order (two calls on
 * the same logits return the same bits), integer atomics on hits only. */
int y2_score_views(const float* logits, const int32_t* labels, int n, int views, int classes, int k, int n_valid,
                   float* prob, int32_t* top_idx, float* top_val, int32_t* rank, int32_t* hits, void* stream);

/* ---- host utility: CRC-32C (Castagnoli) of a host buffer, continuing from `crc` (0 to start).  The checksum of
 *      TensorFlow's V2 checkpoint files (tensor bundle + table blocks), which the reference reads and writes through
 *      tf.train.Saver (src/yolo2_nets/net_utils.py:64-110); used by utils/tf_bundle.py on 100-MB tensors. */
uint32_t y2_crc32c(const void* data, size_t n, uint32_t crc);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
