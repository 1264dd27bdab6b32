/* libshf_hip.so -- C ABI of the MI355X-native detection runtime.
 *
 * This is the drop-in boundary for the reference's inference hot path.  Each entry
 * point names the reference interface it replaces (paths relative to the reference
 * repo bairdzhang/smallhardface).  All functions return 0 on success (or a valid
 * pointer) and non-zero / NULL on failure with a message in shf_last_error();
 * nothing aborts the process (Caffe's glog CHECKs do).
 *
 * Layout contract: host-visible blob data is fp32 NCHW exactly like pycaffe
 * (caffe/python/caffe/_caffe.cpp:222-242); the device keeps activations NHWC.
 */
#ifndef SHF_HIP_H_
#define SHF_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shf_net shf_net;

/* ---- process / device ------------------------------------------------------ */
/* caffe.set_mode_gpu()            caffe/python/caffe/_caffe.cpp:52,394 (set_mode_gpu) */
int shf_set_mode_gpu(void);
/* caffe.set_device(id)            caffe/python/caffe/_caffe.cpp:396 (Caffe::SetDevice) */
int shf_set_device(int device_id);
int shf_device_count(void);
const char* shf_last_error(void);
const char* shf_version(void);

/* ---- Net ------------------------------------------------------------------- */
/* caffe.Net(proto, weights, phase) -- legacy 3-arg ctor, _caffe.cpp:137-151
 * (Net::Net net.cpp:28 + CopyTrainedLayersFrom net.cpp:733).  prototxt_path may
 * be NULL when prototxt_text is given.  caffemodel may be NULL/"" (parameters are
 * then zero until set through shf_net_param_*).  phase: 1 = TEST. */
shf_net* shf_net_create(const char* prototxt_path, const char* prototxt_text,
                        const char* caffemodel_path, int phase);
/* Execution lane: a second net over the SAME parameter tensors (Net::ShareTrainedLayersWith,
 * net.cpp:665-685) with its own activations, workspace and HIP stream, so independent
 * pyramid units overlap on the GPU.  Destroy lanes before the net they were cloned from. */
shf_net* shf_net_clone(shf_net* src);
void shf_net_destroy(shf_net* net);

/* Net._blob_names / Net._inputs / Net._outputs          _caffe.cpp:432-440 */
int shf_net_num_blobs(shf_net* net);
const char* shf_net_blob_name(shf_net* net, int i);
int shf_net_num_inputs(shf_net* net);
int shf_net_input_blob(shf_net* net, int i);   /* index into blobs */
int shf_net_num_outputs(shf_net* net);
int shf_net_output_blob(shf_net* net, int i);
/* Net._layer_names / Layer.type / Layer.blobs           _caffe.cpp:434,483-487 */
int shf_net_num_layers(shf_net* net);
/* classes of the net's proposal layer, background first (proposal_layer.py:118: scores.shape[1] / A): 2 .. 8, taken from
 * the class predictors' output counts; 0 for a net without a proposal layer */
int shf_net_num_classes(shf_net* net);
/* proposal layers ("modules") of the net, 0 .. 4: the driver collects a net's proposals per level from the blobs named
 * boxes_<level> / cls_prob_<level>, one pair per module (lib/test.py:67-83); a net with one module names them boxes /
 * cls_prob.  Every module runs in Net.forward / shf_net_forward_group; the entry points that keep one device list per net
 * (shf_detect_begin / _add_level / _add_levels, shf_class_lists_*, shf_debug_proposal, shf_debug_append) refuse a net with
 * more than one.  0 for a net without a proposal layer */
int shf_net_num_modules(shf_net* net);
const char* shf_net_layer_name(shf_net* net, int i);
const char* shf_net_layer_type(shf_net* net, int i);
int shf_net_layer_num_params(shf_net* net, int layer);
/* shape of param blob `idx` of layer `layer`; returns ndim (<=4) */
int shf_net_param_shape(shf_net* net, int layer, int idx, int* dims);
/* Host pointer to the parameter (Caffe layout: conv (Cout,Cin/g,kh,kw), bias (Cout)).
 * Writing through it and then calling shf_net_param_commit re-packs it on the device
 * (equivalent of writing net.params[name][i].data[...]).  Shared params
 * (param { name: } in the prototxt, net.cpp:421-513) alias one buffer. */
float* shf_net_param_data(shf_net* net, int layer, int idx);
int shf_net_param_commit(shf_net* net, int layer);

/* Blob.reshape(*dims)              _caffe.cpp:244-256 -> Blob::Reshape blob.cpp:23 */
int shf_blob_reshape(shf_net* net, int blob, const int* dims, int ndim);
/* Blob.shape                       _caffe.cpp:455-459; returns ndim */
int shf_blob_shape(shf_net* net, int blob, int* dims);
/* Blob.data -> mutable_cpu_data()  _caffe.cpp:222-242, syncedmem.cpp:39-64:
 * syncs device->host (NHWC->NCHW) if the device copy is newer, marks host as head.
 * The pointer stays valid until the blob grows. */
float* shf_blob_mutable_host_data(shf_net* net, int blob);
/* Blob::set_gpu_data               caffe/src/caffe/blob.cpp:114-121 -> SyncedMemory::set_gpu_data syncedmem.cpp:121-134, with
 * forward_net's pad and detect()'s flip (lib/test.py:35-38,150) folded in: src_dev is an (n, c, h, w) fp32 NCHW contiguous
 * block in DEVICE memory; it lands in the (n, c, H, W) input blob mirrored along x when flip = 1, every element below h /
 * right of w written as +0.0f (csrc/blob_io.hip pad_flip_nchw_kernel, enqueued on the net's stream).  The device copy becomes
 * the blob's head (a later shf_blob_mutable_host_data reads it back).  Refused with a message, before anything is launched:
 * a blob that is not a 4-D net input, a NULL source, n / c other than the blob's, h / w below 1 or above the blob's, flip
 * outside {0, 1}.  The source must be complete when the call is made and stay alive until the net next synchronises. */
int shf_blob_load_device(shf_net* net, int blob, const float* src_dev, int n, int c, int h, int w, int flip);
/* Blob.gpu_data()                  caffe/src/caffe/blob.cpp:108-111 -> SyncedMemory::gpu_data syncedmem.cpp:110-119 (to_gpu
 * :66-91; pycaffe's Blob._gpu_data_ptr, _caffe.cpp:468-470): a DEVICE pointer to the blob's fp32 NCHW image (inputs:
 * uploaded first when the host copy is newer; NHWC activations: transposed into the blob's staging buffer), valid until
 * the next forward, reshape or load on this net.  The net's stream is synchronised before the call returns, so a consumer
 * on any stream may read.  NULL with a message for a tail-fused blob (read those through shf_blob_mutable_host_data), a
 * blob that was never forwarded or written, and a blob with zero elements. */
const float* shf_blob_device_data(shf_net* net, int blob);
/* The same for the SAME input blob of n nets in ONE launch (csrc/blob_io.hip pad_flip_nchw_group_kernel: an image's ten
 * (scale, flip) units are ten such loads, seven of them launch-bound): member i's blob `blob` -- (n_i, c_i, H_i, W_i), its own
 * shape -- receives src_dev[i], an (n_i, c_i, h[i], w[i]) block, mirrored when flip[i] = 1.  members: as for
 * shf_net_forward_group.  The per-member checks and messages of shf_blob_load_device, prefixed "member <i>: "; ALL checks run
 * before anything is allocated or launched, so a refused call changes no member.  The same state changes per member; the
 * copy is enqueued on `net`'s stream (follow with shf_net_forward_group on the same `net`). */
int shf_blob_load_device_group(shf_net* net, int n, shf_net** members, int blob, const float* const* src_dev,
                               const int* h, const int* w, const int* flip);
/* Net._forward(0, n-1)             _caffe.cpp:414 -> Net::ForwardFromTo net.cpp:516 */
int shf_net_forward(shf_net* net);
/* Net::ForwardFromTo (net.cpp:516) for EACH of n nets, run as ONE grouped pass: every convolution, the deconvolution and
 * every stage of the proposal tail is one launch over the group (the walk shf_detect_add_levels runs), whatever the
 * members' spatial sizes -- this is not a batch axis, every member keeps its own shapes and buffers.  members[i] is `net`
 * itself and / or lanes of the same root (shf_net_clone), pairwise distinct, 1 <= n <= 16 (one kernel-argument member
 * table).  `net` is the head of the pass: its stream, range flag and profiler serve it; work enqueued earlier on a member's
 * own stream (shf_blob_load_device) is waited for at entry.  Per member everything shf_net_forward does: shapes re-inferred
 * and buffers grown when the data shape changed, inputs uploaded whose host copy is newer, im_info read from the member's
 * own blob.  On return every member is in the state shf_net_forward(member) would have left it in (output shapes from its
 * own proposal count, every blob readable through shf_blob_mutable_host_data / shf_blob_device_data), its results bit for
 * bit those of a single forward, and the host mirrors of its proposal outputs are already filled (the counts are known
 * here: one synchronisation for the group instead of two read-backs per member).
 * Range guard: a grouped pass has ONE flag.  When it is raised in a split-fp16 mode the WHOLE group is redone on the exact
 * fp32 per-layer kernels -- members that did not overflow are redone too -- and shf_net_range_fallbacks goes up by one.
 * Refused with a message, before anything is allocated or launched: n outside 1..16, a NULL member, duplicate members, a
 * member that does not share `net`'s parameter tensors, a head on which shf_net_set_pipeline is enabled. */
int shf_net_forward_group(shf_net* net, int n, shf_net** members);

/* The in-graph Python layer reads cfg.TEST.{N_DETS_PER_MODULE,SCORE_THRESH,
 * ANCHOR_MIN_SIZE} from the global config (lib/layers/proposal_layer.py:88-92);
 * the native proposal stage takes them here. */
int shf_net_set_proposal_cfg(shf_net* net, int pre_nms_topN, float score_thresh, float min_size);

/* Arithmetic of the MFMA convolutions (3x3 at any dilation and 1x1): 0 = exact fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32, bit-for-bit an fmaf chain); 1 = split-fp16 (2, 3: see the ladder below): x = hi + lo*2^-11 with
 * three fp16 MFMAs per product, fp32 accumulate (2^-22 relative per product: fp32-class, 5.3x
 * the fp32 MFMA rate).  Default 0, or the SHF_CONV_MODE environment variable at creation.  The mode is shared by
 * a net and all lanes cloned from it (like the proposal configuration above). */
int shf_net_set_conv_mode(shf_net* net, int mode);
int shf_net_get_conv_mode(shf_net* net);
/* The reduced-precision ladder (BASELINE configs C3 / C5 name bf16): modes 2 and 3 of shf_net_set_conv_mode form two
 * (a_hi*b_hi + a_hi*b_lo: activations rounded to fp16, weights still split) or one (plain fp16 operands) of the three
 * fp16 products, at 2/3 and 1/3 of the matrix-core work; their score drift against the fp32 reference is measured,
 * not assumed (tools/precision_ladder.py -> profiles/).  shf_net_set_layer_products overrides the count for ONE
 * layer by name (1..3; 0 clears), so a mode can be relaxed only where the measured contribution to the score error is
 * negligible.  Shared by a net and its lanes.  Every split-fp16 kernel (4-wave family, 8-wave, fused first pair) has
 * the 2- and 1-product instantiations; the fused pair's conv1_1 (0.5 % of the FLOPs) always forms three.
 * Mode 4 = bf16: ONE v_mfma_f32_32x32x16_bf16 product per fp32 product, operands rounded to bf16 (8 mantissa bits), fp32
 * accumulate, fp32 activations in HBM.  bf16 has fp32's exponent range: no range guard, no weight refusal.  Like modes 2
 * and 3 it is a drift-labelled throughput mode, not a parity mode (bench.py reports its drift beside the headline).
 * Mode 5 = f64: out = fl32(bias + sum a*w) with the fp32 operands widened to binary64, the products (exact there) and the
 * sum in binary64 on v_mfma_f64_16x16x4_f64, ONE rounding to fp32 -- in every Convolution, the cls / bbox predictors of the
 * tail and the depthwise deconvolution.  Activations stay fp32.  It is the on-device truth the drift of modes 0 and 1 is
 * measured against (tools/precision_ladder.py), not a throughput mode: it always runs layer by layer like mode 0, keeps
 * no packs, has no range guard, and shf_net_set_layer_products has no effect in it. */
int shf_net_set_layer_products(shf_net* net, const char* layer, int nprod);
/* fp16 range guard of mode 1 (the reference is fp32 everywhere, caffe/python/caffe/_caffe.cpp:46-48): hi = fp16(x)
 * overflows above 65504.  Weights are checked when they are packed (shf_net_param_commit / shf_net_set_conv_mode
 * fail with a message).  Every split-fp16 convolution raises a device flag when one of its outputs leaves the range:
 * shf_net_forward then re-runs that forward on the exact fp32 kernels (the count of such re-runs is returned here,
 * shared by a net and its lanes); on the fused path shf_detect_finish / shf_detect_export(_many) fail with
 * "split-fp16 range exceeded ..." so that the caller can re-run the image in mode 0 -- never a silent inf/NaN. */
long long shf_net_range_fallbacks(shf_net* net);
/* (Re)allocations this process has made so far in the runtime's grow-only device / pinned-host buffers (Blob::Reshape
 * semantics, caffe/src/caffe/blob.cpp:22-50: capacity only ever grows; syncedmem.cpp:15-50 is where Caffe allocates).  A
 * stream of images whose shapes were all seen before must leave both counts unchanged.  Measurement only. */
void shf_alloc_counts(long long* device_allocs, long long* pinned_host_allocs);
/* The byte (0..255) that the environment's SHF_POISON_ALLOC made this process fill fresh device allocations with, or -1
 * when the knob is unset.  Parsed once, at first use (strtol base 0: "0xff", "127").  Tests only
 * (tests/test_gpu_buffer_history.py asserts it against its environment, so that the knob cannot be lost unnoticed). */
int shf_debug_poison_byte(void);
/* _get_image_blob (lib/utils/test_utils.py:29-46) + im_list_to_blob (lib/utils/blob.py:16-32) for a whole scale list, for
 * callers that keep HOST blobs (lib/test.py:109-178 detect() -> forward_net): `im_bgr_host` uint8 HxWx3 is uploaded once,
 * level i = mean subtraction + cv2.resize(fx = fy = scales[i], INTER_LINEAR) restated (csrc/pre.hip: the host mirror's
 * arithmetic bit for bit; scale 1.0 = no resize) lands in out_host[i] as an UNPADDED, unflipped (1,3,lvl_h[i],lvl_w[i])
 * fp32 blob; lvl_h / lvl_w from shf_pyramid_level_shape.  The reference calls a native library (OpenCV) at this point too. */
int shf_image_blobs(const uint8_t* im_bgr_host, int im_h, int im_w, int n, const double* scales, const double* pixel_means,
                    float* const* out_host, const int* lvl_h, const int* lvl_w);
/* The same with the levels written straight to caller-owned DEVICE buffers (a torch allocation, say) and nothing copied
 * back: out_dev[i] receives the unpadded, unflipped (1,3,lvl_h[i],lvl_w[i]) fp32 blob.  Same argument checks, same kernel,
 * same stream; synchronised before the call returns.  Feed the levels to a net with shf_blob_load_device. */
int shf_image_blobs_device(const uint8_t* im_bgr_host, int im_h, int im_w, int n, const double* scales,
                           const double* pixel_means, float* const* out_dev, const int* lvl_h, const int* lvl_w);
/* PCI bus id ("0000:c5:00.0") of the device the runtime is set to (shf_set_device; caffe.set_device,
 * caffe/python/caffe/_caffe.cpp:394-396), so that a host-side sampler can find the card's sysfs hwmon files (clock, socket
 * power) without a GPU call of its own.  Measurement only (bench.py `telemetry`). */
int shf_device_pci_bus_id(char* out, int cap);

/* ---- fused per-image path (device-resident pyramid; lib/test.py:109-178) ---- */
/* detect(): begin an image */
int shf_detect_begin(shf_net* net);
/* forward_net() for one (scale, flip) unit, lib/test.py:21-66: `data` is the level
 * blob (1,3,H,W) fp32 NCHW already padded to MAX_RESOLUTION, on the device when
 * data_on_device != 0; im_h/im_w are the UNPADDED dims that go to im_info and
 * the flip fix; detections with fg prob > thresh are un-flipped, unscaled and
 * appended to the image's device-side list (test.py:52-54,59-66,163-167). */
int shf_detect_add_level(shf_net* net, const float* data, int data_on_device,
                         int H, int W, int im_h, int im_w, float im_scale, int flip, float thresh);
/* The same for a GROUP of units at once (the whole pyramid of an image): every MFMA conv
 * layer runs as ONE grid over all units (they share the layer's weights, not the spatial
 * size), so the small levels do not serialise latency-bound launches.  members[i] supplies
 * the activation buffers of unit i: `net` itself and/or lanes made with shf_net_clone, all
 * distinct, at most 16 per call (one kernel-argument member table; more units = several calls, the lists
 * concatenate); the work is enqueued on `net`'s stream and the detections land in `net`'s image
 * list in unit order -- or, with per_member_lists != 0 (units of DIFFERENT images, the multi-GPU
 * window), in each member's own list (reset first); synchronise `net` before exporting them. */
int shf_detect_add_levels(shf_net* net, int n, shf_net** members, const float* const* data,
                          int data_on_device, const int* H, const int* W, const int* im_h,
                          const int* im_w, const float* im_scale, const int* flip, float thresh,
                          int per_member_lists);
/* ---- image pre-processing ----------------------------------- */
/* Geometry of one pyramid unit: the resized level is (lvl_h, lvl_w) = round-half-even(im * scale)
 * (cv2.resize dsize rule, lib/utils/test_utils.py:40-44) and the net input (H, W) is that rounded
 * up to a multiple of max_resolution (cfg.MAX_RESOLUTION, lib/test.py:35-38).  Needs no GPU. */
int shf_pyramid_level_shape(int im_h, int im_w, double scale, int max_resolution, int* lvl_h, int* lvl_w,
                            int* H, int* W);
/* _get_image_blob for one (scale, flip) unit on the device (lib/utils/test_utils.py:29-46,
 * lib/utils/blob.py:16-32, flip lib/test.py:150, pad lib/test.py:35-38): im_bgr_dev is the raw
 * im_h x im_w x 3 uint8 image (cv2.imread layout) in device memory, pixel_means 3 doubles
 * (cfg.PIXEL_MEANS), out_dev receives the (1,3,H,W) fp32 blob forward_net would build, H/W/lvl_*
 * from shf_pyramid_level_shape.  Enqueued on `net`'s stream; pass out_dev to
 * shf_detect_add_level(s) with data_on_device = 1. */
int shf_make_pyramid_level(shf_net* net, const uint8_t* im_bgr_dev, int im_h, int im_w, double scale, int flip,
                           const double* pixel_means, float* out_dev, int H, int W, int lvl_h, int lvl_w);
/* Cross-lane ordering for software-pipelining images over two head lanes: record marks the
 * current end of `net`'s stream; wait makes `net`'s stream wait for `other`'s last mark (e.g. the
 * next image's convolutions, which reuse the member lanes' buffers, wait for the previous
 * image's appends while its box merging still runs). */
int shf_net_record_event(shf_net* net);
int shf_net_wait_event(shf_net* net, shf_net* other);
/* Finer hand-over for the same pipeline: with `prev` set as `net`'s predecessor head,
 * shf_detect_add_levels on `net` starts its convolutions as soon as the member lanes' previous tails
 * have consumed the head feature maps (their logits kernels), and waits for `prev`'s last
 * shf_net_record_event mark only before its own tails, which reuse the members' tail buffers.
 * prev = NULL clears it. */
int shf_net_set_predecessor(shf_net* net, shf_net* prev);
/* Image pipeline over head lanes, robust form: with enable != 0 the grouped passes of `net` put their convolutions
 * and logits kernels on ONE in-order stream shared by the net and all its lanes (consecutive images queue behind
 * each other, no cross-stream hand-over of the activation buffers), and only the rest of the tails, the appends and
 * the merge run on `net`'s own stream, which is re-created with the highest stream priority so that its tiny kernels
 * are dispatched beside the next image's convolutions.  Combine with shf_net_set_predecessor (the members' tail
 * workspaces are handed from head to head). */
int shf_net_set_pipeline(shf_net* net, int enable);
/* Box merging for the image (test.py:168-175): method 0 = BBOX_VOTE (test.py:181),
 * 1 = NMS (lib/nms).  out5 rows are (x1,y1,x2,y2,score) as double (bbox_vote
 * returns float64).  *n_out = number of rows (may exceed cap; only cap written). */
int shf_detect_finish(shf_net* net, int method, float nms_thresh, double* out5, int cap, int* n_out);
/* number of >thresh detections gathered so far for the current image */
int shf_detect_count(shf_net* net);
/* Pyramid sharding across GPUs (the reference gathers per-worker results through a
 * multiprocessing.Queue, lib/test.py:327-344; here units of ONE image may live on several
 * GPUs): export copies the current image's (x1,y1,x2,y2,score) fp32 rows to a caller-owned
 * DEVICE buffer (for an RCCL gather); import appends rows gathered from other ranks (device
 * pointer) to the current image before shf_detect_finish. */
int shf_detect_export(shf_net* net, float* dst_dev5, int cap_rows, int* n_rows);
int shf_detect_import(shf_net* net, const float* src_dev5, int n_rows);
/* export of all the per-member lists of one shf_detect_add_levels(..., per_member_lists=1) pass */
int shf_detect_export_many(shf_net* net, int n, shf_net** members, float* const* dst_dev5, int cap_rows,
                           int* n_rows);

/* ---- per-class detection lists of a multi-class image (csrc/class_lists.hip) ----
 * What detect() does on the host after its forwards, for a net with C classes (2 .. 8), on the device: the per-unit flip
 * fix and unscale of forward_net (lib/test.py:52-66), the per-class > thresh cut (lib/test.py:161-167) and the per-class
 * merge (:168-176).  `net` -- the head -- holds C - 1 lists of (x1, y1, x2, y2, score) fp32 rows, one per foreground
 * class; they stay in HBM from the proposal layer's outputs to the merged boxes.  The lists are separate from the
 * single-list fused path (shf_detect_*), whose refusal of C > 2 stands.  Every entry below refuses, by name and before
 * anything is launched: a NULL net or argument, a net without a proposal layer, a head with shf_net_set_pipeline
 * enabled, and cls outside 1..C-1 where a class is named.
 *
 * begin: empties the lists (lib/test.py:131-132, the empty all_probs / all_boxes). */
int shf_class_lists_begin(shf_net* net);
/* add (lib/test.py:52-66 per unit, :161-167 the cut): appends the outputs of n members, 1 <= n <= 16, each of which has
 * completed a forward (shf_net_forward / shf_net_forward_group), read where they sit in the members' `boxes` / `cls_prob`
 * device buffers; R is the row count the member's last forward recorded (a member whose proposal layer emitted only the
 * dummy roi has R = 0 and contributes nothing).  Member i's boxes are mirrored about im_w[i] when flip[i] != 0, then
 * divided by im_scale[i] (fp32 division).  List c - 1 receives every row with cls_prob[r, c] > thresh in (member, row)
 * order -- np.where on the concatenated units -- behind the rows it already holds: a later group of the same image
 * continues the lists.  Positions come from prefix sums, never from atomics.  A list holds at most units x rmax rows
 * (rmax = cfg.TEST.N_DETS_PER_MODULE, or the anchor count when that is <= 0; the buffers grow to at least 16 x rmax):
 * rows beyond that are dropped and the length is clamped.  Runs on `net`'s stream.  Also refused: n outside 1..16, a
 * member without a completed forward, a member whose class count differs from the head's. */
int shf_class_lists_add(shf_net* net, int n, shf_net** members, const int* im_w, const float* im_scale, const int* flip,
                        float thresh);
/* diagnostics: the same with HOST arrays injected in place of forwarded members (cf. shf_debug_append): boxes5[i] (R[i],5)
 * and probs[i] (R[i],C) fp32, C = shf_net_num_classes(net); boxes5[i] / probs[i] may be NULL when R[i] == 0. */
int shf_debug_class_lists_add(shf_net* net, int n, const float* const* boxes5, const float* const* probs, const int* R,
                              const int* im_w, const float* im_scale, const int* flip, float thresh);
/* counts[0 .. C-2] = rows of each list (synchronises `net`'s stream) */
int shf_class_lists_count(shf_net* net, int* counts);
/* the rows of class cls (1 .. C-1) to a caller-owned DEVICE buffer of cap_rows rows, as shf_detect_export does for the
 * single list; returns the list's row count (which may exceed cap_rows: only cap_rows are written), -1 on error */
int shf_class_lists_export(shf_net* net, int cls, float* dst_dev5, int cap_rows);
/* the merge of class cls (lib/test.py:168-176) on the device: method / nms_thresh / out5 / cap / n_out as
 * shf_detect_finish.  An empty class under BBOX_VOTE gives the row (10, 10, 20, 20, 0.0001) (lib/test.py:184-186); under
 * NMS the rows are dets[keep] in keep order, none for an empty class.  More than 262144 rows in the class are refused
 * like every merge. */
int shf_class_lists_finish(shf_net* net, int cls, int method, float nms_thresh, double* out5, int cap, int* n_out);

/* ---- stand-alone box ops ----------------------------------------------------- */
/* nms(dets, thresh)  lib/nms/nms_wrapper.py:13 -> gpu_nms lib/nms/gpu_nms.pyx:16-31
 * -> _nms lib/nms/gpu_nms.hpp:1 (nms_kernel.cu:102-155).  Takes UNSORTED dets
 * (n,5) fp32 host memory and returns indices into it, score-descending, like
 * gpu_nms.pyx:31 (`order[keep]`).  Suppression predicate IoU > thresh
 * (nms_kernel.cu:82).  keep must hold n ints. */
int shf_nms(const float* dets5, int n, float thresh, int device_id, int32_t* keep, int* n_keep);
/* bbox_vote(det)     lib/test.py:181-217, thresh = cfg.TEST.NMS_THRESH.
 * dets5 (n,5) fp32 host; out5 (cap,5) double. */
int shf_bbox_vote(const float* dets5, int n, float thresh, double* out5, int cap, int* n_out);
/* generate_anchors() lib/layers/generate_anchors.py:11-24; out (n_ratios*n_scales*n_shifts^2, 4) */
int shf_generate_anchors(int base_size, const double* ratios, int n_ratios, const double* scales,
                         int n_scales, const double* shifts, int n_shifts, const double* strides,
                         double* out, int cap_rows);

/* image_eval + img_pr_info + dataset_pr_info   lib/wider_eval_tools/wider_eval.py:62-130, for all images and up to 8
 * settings (easy / medium / hard subsets of the same ground truth) in one call, on the current device.
 *   pred5     (N,5) x, y, w, h, score; the rows of image i are pred_off[i] .. pred_off[i+1] (n_images + 1 offsets) and
 *             score-descending; the scores are compared as given (the caller normalises them, wider_eval.py:42-59)
 *   gt4       (G,4) x, y, w, h with gt_off alike; counted (n_settings, G): 1 where the box belongs to the setting's subset
 *   thresh    n_thresh score thresholds as the caller computes them (1 - (t + 1) / 1000, wider_eval.py:109)
 *   totals    (n_settings, n_thresh, 2): over all images, the number of proposals and of subset faces found with
 *             score >= thresh -- exact integers, the sums dataset_pr_info forms
 *   hits_out / proposal_out   (n_settings, N) each, or NULL (diagnostics, tests): per detection the number of subset
 *             faces found so far in its image, and 0 where it sits on a face outside the subset (proposal_list = -1)
 * A detection is attributed to the FIRST ground-truth box with the largest IoU (fp64, +1 pixel convention, zero-union
 * guard :62-79), with mimic_eval_bug != 0 the largest floor(IoU + 0.5) (:92-95), and matched when that value is
 * >= iou_thresh.  All buffers are host memory.  Images without detections or without ground truth contribute nothing.
 * Refused with a message, before anything is allocated or launched: negative or non-monotone offsets, iou_thresh outside
 * (0, 1], n_settings outside 1..8, n_settings x N or n_settings x G of 2^31 rows or more, an image with more than
 * 65 536 ground-truth boxes (one lane walks them all).  Non-finite boxes or scores are the caller's to keep away
 * (numpy's arg-max of NaN is not reproduced). */
int shf_wider_eval_counts(const double* pred5, const int* pred_off, const double* gt4, const int* gt_off,
                          const uint8_t* counted, int n_images, int n_settings, double iou_thresh, int mimic_eval_bug,
                          const double* thresh, int n_thresh, long long* totals, int* hits_out, uint8_t* proposal_out);

/* One matching round of the AFW / Pascal Faces evaluator, for all images in one call, on the current device:
 * VOCprRecordOptim  external/marcopede-face-eval-f2870fd85d48/VOCpr.py:118-162 with the IoU of util.overlap
 * (util.py:176-193: abs() extents + 1, a strict > intersection test, ia / (a1 + a2 - ia) in fp64, that operation order).
 *   det4       (N,4) x1, y1, x2, y2; the rows of image i are det_off[i] .. det_off[i+1] (n_images + 1 offsets), in the
 *              evaluator's global score-descending order (grouping by image keeps all the matching depends on)
 *   gt4        (G,4) x1, y1, x2, y2 with gt_off alike; difficult (G): non-zero where the box is "difficult"
 *   code_out   (N) 0 = neither (the best box is difficult), 1 = true positive, 2 = false positive
 *   index_out  (N) the chosen box counted within its image, -1 for an image without boxes
 * The chosen box is the LAST one holding the largest IoU (the reference compares covr >= maxovr, from maxovr = 0 and
 * index 0).  True positive: IoU > ovr (strict) on a box that is not difficult and that no earlier detection of the call
 * has taken; false positive: the box is taken, or IoU <= ovr, or the image has no boxes.  Integers only: translations,
 * means, the refinement transform, the curve and the AP stay with the caller, one call per refinement round.
 * All buffers are host memory.  Refused with a message, before anything is allocated or launched: negative or
 * non-monotone offsets, ovr outside (0, 1], 2^31 rows or more of either kind.  Non-finite boxes are the caller's to keep
 * away (Python's comparison chain on NaN is not reproduced). */
int shf_face_eval_match(const double* det4, const long long* det_off, const double* gt4, const long long* gt_off,
                        const uint8_t* difficult, int n_images, double ovr, int* code_out, int* index_out);

/* The pixel counts of the FDDB evaluator (smallhardface_amd/fddb_eval.py), for all images in one call, on the current
 * device: per (annotation, detection) pair of an image the pixels inside both masks, and per annotation its area.
 * Masks live on integer pixel coordinates (ix, iy):
 *   rectangle  rint(x) <= ix <= rint(x + w), rint(y) <= iy <= rint(y + h), both corners inclusive, cut to the canvas
 *              0 <= ix < W, 0 <= iy < H when the image size is known.  The CALLER rounds and cuts: rect4 holds integers.
 *   ellipse    with c = cos(angle), s = sin(angle) SUPPLIED BY THE CALLER (computed once on the host; the device calls no
 *              sin or cos), dx = ix - cx, dy = iy - cy, u = dx*c + dy*s, v = dy*c - dx*s the pixel is inside when
 *              (u*u)*(rb*rb) + (v*v)*(ra*ra) <= (ra*ra)*(rb*rb): fp64 in exactly that operation order, no contraction.
 *   ell6       (A,6) ra, rb, c, s, cx, cy; the rows of image i are ann_off[i] .. ann_off[i+1] (n_images + 1 offsets)
 *   ell_box    (A,4) x0, y0, x1, y1: the inclusive integer scan box of each ellipse -- its bounding box, taken generously,
 *              cut to the canvas; empty when x1 < x0 or y1 < y0.  Only pixels of the box are tested.
 *   rect4      (D,4) x0, y0, x1, y1 inclusive, with det_off alike; empty when x1 < x0 or y1 < y0
 *   inter_out  image i's (A_i, D_i) counts, row-major, at the sum of A_j * D_j over j < i: pixels of
 *              rect n scan box that pass the ellipse test
 *   area_out   (A) pixels of the scan box that pass the ellipse test
 * Integers only: rectangle areas, the scores, the assignment and the curves stay with the caller.  All buffers are host
 * memory.  Refused with a message, before anything is allocated or launched: null offsets, negative or non-monotone
 * offsets, 2^31 rows or more of either kind, 2^26 (annotation, detection) pairs or more (one 64-lane block per pair, in one
 * launch), null arrays with non-zero counts, a corner of 2^30 or more in magnitude, a scan
 * box of more than 1 048 576 pixels (2^20: one wave sweeps a box 64 pixels at a time, the cap bounds how long it runs;
 * FDDB's images are under 500 pixels a side, so any real face passes).  Non-finite parameters are the caller's to keep
 * away.
 *   phase_ms   NULL, or 3 doubles (measurement): the milliseconds the call's stream spent on the uploads, the kernels and
 *              the read-back, from events on that stream; zeros when nothing was launched */
int shf_fddb_pair_counts(const double* ell6, const int* ell_box, const long long* ann_off, const int* rect4,
                         const long long* det_off, int n_images, int* inter_out, int* area_out, double* phase_ms);

/* Read parameter blob `idx` of layer `layer` from a binary .caffemodel (the reader behind
 * shf_net_create's weight loading; caffe.proto NetParameter.layer=100 / BlobProto data=5).
 * Returns the element count (out may be NULL to query), fills dims/ndim.  Needs no GPU. */
int shf_caffemodel_read_blob(const char* path, const char* layer, int idx, float* out, int cap,
                             int* dims, int* ndim);

/* ---- diagnostics (tests) ------------------------------------------------------ */
/* the hand-over event a later pass over `net` as a member lane would wait for (set by the fused passes): *waits = 1 when
 * there is one, *holds = 1 when `net` itself keeps that event alive -- its own event, or a share of the head's whose
 * grouped pass set it.  A lane that waits for an event it does not hold would wait on a destroyed one once that head is
 * gone. */
int shf_debug_handover_event(shf_net* net, int* waits, int* holds);
/* runs the merge pipeline on host dets and returns its intermediates: the IoU bit matrix
 * (n x ceil(n/64) words, upper triangle), cluster head per box, kept heads, sorted dets, perm */
int shf_debug_merge(const float* dets5, int n, float thresh, int ge_pred, unsigned long long* mask_out,
                    int* cluster_out, int* heads_out, int* n_heads, float* sorted_out, int* perm_out);

/* The proposal stage alone -- tail decode -> candidate select -> sort -> gather -- on INJECTED blobs, so the
 * reference's own ProposalLayer.forward vectors (lib/layers/proposal_layer.py:60-220, incl. the
 * np.seterr(over='raise') clamp branch of lib/utils/bbox_transform.py:52-65) reach the HIP kernels: scores =
 * cls_prob_reshape_output (1,C*A,h,w) with channel c*A + a, deltas = bbox_pred_output (1,4A,h,w), im_info3 =
 * (h, w, scale), all host fp32.  Anchors, the class count C (shf_net_num_classes) and cfg.TEST.* come from `net` (any
 * net holding the proposal layer).  out_boxes5 (cap,5) / out_probs2 (cap,C) receive the layer's tops: *n_out = R rows,
 * ranked by the best foreground class (when R == 0 out_boxes5 holds the dummy roi); *overflow != 0 when the clamp branch
 * was taken. */
int shf_debug_proposal(shf_net* net, const float* scores, const float* deltas, int h, int w, const float* im_info3,
                       float* out_boxes5, float* out_probs2, int cap, int* n_out, int* overflow);
/* forward_net's flip fix + unscale (lib/test.py:52-54,59-66) and detect()'s > thresh cut (:163-167) on injected
 * proposals boxes5 (R,5) / probs2 (R,2) (host, score-descending like the layer emits them): appended to the
 * current image's device list as one more unit (after shf_detect_begin; read back with shf_detect_export).
 * The per-image lists (this call, shf_detect_begin, shf_detect_add_level(s)) hold one foreground class: a net with
 * more than two classes is refused, with the class count in the message, before anything is launched. */
int shf_debug_append(shf_net* net, const float* boxes5, const float* probs2, int R, int im_w, float im_scale,
                     int flip, float thresh);

/* ---- measurement ------------------------------------------------------------- */
/* Per-kernel-class HIP-event timing on the net's stream.  enable!=0 starts recording
 * an event pair around every launch; shf_prof_read drains them (synchronises) and
 * returns, for class `cls`, the number of launches, total ms and algorithmic FLOPs. */
int shf_prof_enable(shf_net* net, int enable);
/* Restrict the bracketing to launches of ONE class (cls < 0: every class again).  An event pair around a launch costs the
 * stream a few microseconds; bench.py surveys every class in an untimed pass and brackets only the dominant kernel inside
 * its timed region (measured: 79.5 images/s with every launch bracketed, 82.3 with none). */
int shf_prof_only(shf_net* net, int cls);
int shf_prof_num_classes(shf_net* net);
const char* shf_prof_class_name(shf_net* net, int cls);
int shf_prof_read(shf_net* net, int cls, int64_t* launches, double* total_ms, double* flops, double* bytes);
int shf_prof_reset(shf_net* net);
/* Calibration of the roofline's MFMA bound on the box at hand: the issued TFLOP/s a pure stream of
 * v_mfma_f32_32x32x16_f16 (bf16 != 0: _bf16) sustains with the convolution kernels' register diet (one wave per SIMD,
 * 8 accumulator tiles, 3 products per fragment pair) and NO memory traffic, for operands with random signs and
 * mantissas of which zero_eighths/8 of the activation fragments are zero (constant_operands != 0: every element 1.0 --
 * the nominal-peak case).  The chip is power-limited under matrix load and the limit depends on the operands' bit
 * toggling, so this -- not the 2.5 PFLOP/s of non-toggling operands -- is what a kernel that moved its bytes for free
 * could reach.  Runs (reps + 1) / 2 settling launches, then times `reps` launches of `iters` x 24 MFMAs per wave on a
 * private stream; synchronises.  No counterpart in the reference (measurement only). */
int shf_calib_matrix_pipe(int bf16, int zero_eighths, int constant_operands, int iters, int reps, double* tflops);
/* Diagnostics (tests only): the launches the split-fp16 planner gives a 3x3 / pad 1 / dilation 1 convolution cin -> cout
 * on one (1, h, w) unit -- in_split: its input is in the split activation format; pooled: a 2x2 max-pool is fused.
 * Nothing is launched; no GPU is needed.  Per launch (at most two): the dynamic LDS it requests, its grid, and whether it
 * runs the slim three-blocks-per-CU form of the 4-wave kernel.  Returns the number of launches, -1 with a message. */
int shf_debug_conv_plan(int cin, int cout, int h, int w, int in_split, int pooled, long long* lds_bytes, long long* grid_blocks,
                        int* slim);
/* Diagnostics (tests only): the same for a grouped pass over n units (b[i], h[i], w[i]), n <= 16 (b NULL: one image each), planned for `cus` compute
 * units (0: SHF_CONV_CUS, or the device's count).  first_pair != 0: the plan of conv1_2 fused with conv1_1 (cin = cout =
 * 64) instead of a dual-tile family layer.  launches[8 * i ..] of launch i (at most two): grid, dynamic LDS bytes, tile
 * rows, pixel tiles per block, tile_base (the first pixel tile of the launch), ntile_blocks (as the kernel receives it),
 * slim form (0 / 1), persistent first pair (0 / 1); *pc_tab: the persistent pair keeps its per-block tile table (0 / 1).
 * Nothing is launched; no GPU is needed.  Returns the number of launches, -1 with a message. */
int shf_debug_conv_plan_group(int n, const int* b, const int* h, const int* w, int cin, int cout, int in_split, int pooled, int first_pair,
                              int cus, long long* launches, int* pc_tab);
/* stream synchronise (end of a timed region) */
int shf_net_sync(shf_net* net);

#ifdef __cplusplus
}
#endif
#endif /* SHF_HIP_H_ */
