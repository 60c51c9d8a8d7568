/*
 * cim_hip.h - C ABI of libcim_hip.so, the MI355X (gfx950) kernel library behind the
 * per-image training step of ZechengLi19/CIM.
 *
 * Conventions (every entry point):
 *   - returns 0 on success, a positive hipError_t on a HIP failure, -1 on bad arguments;
 *     cim_last_error() returns a thread-local description of the last failure;
 *   - every pointer is a caller-owned DEVICE pointer to a dense array of the stated dtype
 *     (the Python host passes torch.Tensor.data_ptr()); nothing is allocated or freed (no hipMalloc, no events, no streams:
 *     device scratch, fork / join events and side streams are the caller's and come in as arguments), no host synchronisation
 *     happens, no state is kept between calls (no process-wide or per-thread switches, counters or pools): the library is
 *     re-entrant - host threads may call it concurrently on different streams (tests/test_gpu_reentrant.py);
 *     the only per-thread datum is the message behind cim_last_error();
 *   - the last argument is the hipStream_t to launch on, passed as void*
 *     (torch.cuda.current_stream().cuda_stream);
 *   - "f16" arrays hold IEEE binary16 bit patterns (uint16_t).  Python-float thresholds are
 *     rounded to binary16 inside the library before comparing against f16 maps, which is
 *     what the reference's fp16-tensor-vs-Python-scalar compares do.
 *
 * Each entry cites the reference interface it replaces (paths under /root/reference).
 */
#ifndef CIM_HIP_H
#define CIM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* cim_last_error(void);
int cim_abi_version(void);

/* ------------------------------------------------------------------ ROIAlign (a-1, a-2 prologue)
 * Replaces mmcv.ops.RoIAlign(output_size=P, spatial_scale, sampling_ratio, 'avg', aligned)
 * as imported by lib/ops/__init__.py:6 and called at lib/modeling/model_builder.py:229-231
 * (forward) and by autograd (backward).  Arithmetic: SURVEY.md App. D.
 *
 * Layout is channels-last: feat [B,H,W,C] f32, rois [K,5] f32 = (batch, x1, y1, x2, y2) in
 * input-image pixels, out [K,P,P,C] f32.  (The Python wrapper exposes these as logical NCHW
 * tensors in torch.channels_last memory format, so the reference's NCHW API is unchanged.)
 */
int cim_roi_align_fwd(const float* feat, const float* rois, float* out,
                      int B, int C, int H, int W, int K, int P,
                      float spatial_scale, int sampling_ratio, int aligned, void* stream);

/* grad_in [B,H,W,C] is fully overwritten (zero-filled on `stream`, then accumulated).
 * workspace: optional device scratch of cim_roi_align_bwd_workspace(K,P,H,W) bytes; when given, the
 * per-ROI interpolation tables are built once per launch instead of once per (ROI, channel chunk). */
long long cim_roi_align_bwd_workspace(int K, int P, int H, int W);
int cim_roi_align_bwd(const float* grad_out, const float* rois, float* grad_in,
                      int B, int C, int H, int W, int K, int P,
                      float spatial_scale, int sampling_ratio, int aligned, float* workspace, void* stream);

/* Forward with the backward's table workspace (cim_roi_align_bwd_workspace bytes).  Where the geometry takes a table form
 * (CIM_ROI_FWD_ROWSUM2 / CIM_ROI_FWD_AGG below) the per-ROI separable weight tables are built into the workspace once and
 * every bin reads each pixel it touches ONCE with the aggregated weight WY[ph][y]*WX[pw][x]/count - (gh+1)(gw+1) instead
 * of 4*gh*gw loads per bin.  Same result up to the reassociation of the sum (a few ulp; cim_roi_align_fwd keeps the
 * reference's sample order bit for bit).  Any other geometry takes the sample-order kernel and leaves the workspace
 * unwritten.  workspace == NULL behaves like cim_roi_align_fwd / cim_roi_align_maskcat_fwd. */
int cim_roi_align_fwd_ws(const float* feat, const float* rois, float* out,
                         int B, int C, int H, int W, int K, int P,
                         float spatial_scale, int sampling_ratio, int aligned, float* workspace, void* stream);
int cim_roi_align_maskcat_fwd_ws(const float* feat, const float* rois, const float* masks, float* cat,
                                 int B, int C, int H, int W, int K, int P,
                                 float spatial_scale, int sampling_ratio, int aligned, float* workspace, void* stream);

/* Backward with tables_ready != 0: `workspace` is the one a *_fwd_ws call on the SAME rois / geometry was given; the
 * backward reuses the tables in it only where that forward built them (a table form: cim_roi_align_forms) and builds them
 * itself otherwise.  0 always rebuilds them.
 * scratch: cim_roi_align_bwd_scratch(K,B,C,H,W) bytes (0: none needed) for the per-ROI-group partial maps of the
 * region-form backward, which are then summed by one streaming pass; with scratch == NULL the groups meet in
 * grad_in through float atomics (device-scope float atomics run at ~90 G/s on MI355X: 2-3x slower end to end). */
long long cim_roi_align_bwd_scratch(int K, int B, int C, int H, int W);
int cim_roi_align_bwd_ws(const float* grad_out, const float* rois, float* grad_in,
                         int B, int C, int H, int W, int K, int P,
                         float spatial_scale, int sampling_ratio, int aligned, float* workspace, int tables_ready,
                         float* scratch, void* stream);
int cim_roi_align_maskcat_bwd_ws(const float* grad_cat, const float* rois, const float* masks, float* grad_in,
                                 int B, int C, int H, int W, int K, int P,
                                 float spatial_scale, int sampling_ratio, int aligned, float* workspace, int tables_ready,
                                 float* scratch, void* stream);

/* Fused ROIAlign + mask multiply + channel concat: the input of MaskFuse.mask_branch,
 * lib/modeling/resnet50.py:121-134 (vgg16.py:162-175, HRNet.py:615-628):
 *   cat[k,ph,pw,0:C]  = roi_align(feat)[k,ph,pw,:]
 *   cat[k,ph,pw,C:2C] = roi_align(feat)[k,ph,pw,:] * masks[k,ph,pw]
 * masks [K,P,P] f32; cat [K,P,P,2C] f32.  box_x / mask_x are never materialised. */
int cim_roi_align_maskcat_fwd(const float* feat, const float* rois, const float* masks, float* cat,
                              int B, int C, int H, int W, int K, int P,
                              float spatial_scale, int sampling_ratio, int aligned, void* stream);

/* ROIAlign + mask multiply + channel concat + the Winograd INPUT TRANSFORM of MaskFuse.mask_branch's 3 x 3 convolution in one
 * launch (+ the table launch): lib/modeling/resnet50.py:121-135 up to the convolution's contraction.  Writes the pair image
 *   V [121][Rs][2C]  (mixed 4 + 3 tiling of the 7 x 7 map, cim_wino7_input_pair's layout; rows K .. Rs-1 zero; `scale` [121] from
 *   cim_wino7_pair_scales(kind 0))
 * that cim_gemm_pair_batched contracts with the filter image - `cat` is never stored (the two calls cim_roi_align_maskcat_fwd_ws
 * + cim_wino7_input_pair wrote and re-read its 4 * K * 49 * 2C bytes).  Bit-identical to those two calls.  P == 7, C % 8 == 0,
 * H, W <= 128; workspace: cim_roi_align_bwd_workspace(K,P,H,W) bytes, left holding the tables for cim_roi_align_bwd_ws /
 * cim_roi_align_maskcat_bwd_ws (tables_ready = 1: these geometries are a table form of the forward, ROWSUM2). */
int cim_roi_align_wino7_pair_fwd(const float* feat, const float* rois, const float* masks, void* V, const float* scale,
                                 int B, int C, int H, int W, int K, int Rs, int P, float spatial_scale, int sampling_ratio,
                                 int aligned, float* workspace, void* stream);

int cim_roi_align_maskcat_bwd(const float* grad_cat, const float* rois, const float* masks, float* grad_in,
                              int B, int C, int H, int W, int K, int P,
                              float spatial_scale, int sampling_ratio, int aligned, float* workspace, void* stream);

/* Kernel forms of the ROIAlign calls above (ABI-16 addition: cim_abi_version() stays 16).  Host only: no device work.
 * For a geometry - maskcat != 0 for the mask-cat entry points, has_workspace != 0 when a table workspace is passed,
 * tables_ready as given to the backward - it writes the forward kernel the fwd entry points take, the backward kernel
 * the bwd entry points take, and 1 / 0 whether that backward builds the per-ROI tables itself.  The forward builds
 * the tables exactly when its form is ROWSUM2 or AGG.  (K == 0 launches no forward kernel.)  Limits, DESIGN.md 4.3:
 *   forward   ROWSUM2   workspace, C % 4 == 0, H W C < 2^30, H <= 64 or (P >= 4 and H <= 128); P <= 7 and W <= 128
 *             AGG       the same table conditions with P <= 8; P == 8 or W > 128.  A bin row with more than 64 map rows
 *                       or a bin with more than 64 (row, column) entries falls back to the sample order in the kernel.
 *             SAMPLE4   otherwise, C % 4 == 0: the reference's sample order, bit-identical to it
 *             SAMPLE1   otherwise
 *   backward  REGION    K > 0, workspace, C % 4 == 0, P <= 16, H < 256, W < 256, at most 256 regions of 12 x 16 pixels,
 *                       its LDS <= 158 KiB (P = 16 only with 64-ROI groups), K P P C (2C mask-cat) < 2^31
 *             GENERIC4  otherwise, C % 4 == 0: the reference's scatter through global atomics
 *             GENERIC1  otherwise */
#define CIM_ROI_FWD_SAMPLE1 0      /* roi_align_fwd_kernel<1> */
#define CIM_ROI_FWD_SAMPLE4 1      /* roi_align_fwd_kernel<4> */
#define CIM_ROI_FWD_ROWSUM2 2      /* roi_tables_kernel + roi_align_fwd_rowsum2_kernel */
#define CIM_ROI_FWD_AGG 3          /* roi_tables_kernel + roi_align_fwd_agg_kernel */
#define CIM_ROI_BWD_GENERIC1 0     /* roi_align_bwd_kernel<1> */
#define CIM_ROI_BWD_GENERIC4 1     /* roi_align_bwd_kernel<4> */
#define CIM_ROI_BWD_REGION 2       /* roi_align_bwd_region_kernel (+ roi_partial_reduce_kernel: several ROI groups, scratch) */
int cim_roi_align_forms(int B, int C, int H, int W, int K, int P, int maskcat, int has_workspace, int tables_ready,
                        int* fwd_form, int* bwd_form, int* bwd_builds_tables);

/* ------------------------------------------------------------------ RoIPool (FAST_RCNN.ROI_XFORM_METHOD = RoIPoolF)
 * Replaces mmcv.ops.RoIPool(output_size=P, spatial_scale) as imported by lib/ops/__init__.py:6 and called at
 * lib/modeling/model_builder.py:227-228, and - the mask-cat forms - the prologue of MaskFuse.forward behind it
 * (lib/modeling/resnet50.py:131-134).  csrc/roi_pool.hip; DESIGN.md 4.24.  Additive: cim_abi_version() stays 16.
 *
 * Channels-last like ROIAlign: feat [B,H,W,C] f32, rois [K,5] f32 = (batch, x1, y1, x2, y2), out [K,P,P,C] f32,
 * cat [K,P,P,2C] f32, masks [K,P,P] f32, argmax [K,P,P,C] int32.
 *
 * The contract (tests/golden/roi_pool_np.py restates it float for float; out and argmax are bit-identical to it).  All in
 * fp32, every operation rounded separately - no FMA contraction, a correctly rounded division, no reciprocal:
 *   b   = (int) rois[k][0]
 *   rx1 = x1 * s;  ry1 = y1 * s;  rx2 = (x2 + 1) * s;  ry2 = (y2 + 1) * s;  rw = rx2 - rx1;  rh = ry2 - ry1
 *   rw <= 0 or rh <= 0:  every output of the ROI is 0 and every argmax -1
 *   bw = rw / P;  bh = rh / P
 *   bin (ph, pw):  x in [floor(pw * bw + rx1), ceil((pw + 1) * bw + rx1)),  y in [floor(ph * bh + ry1), ceil((ph + 1) * bh + ry1)),
 *                  each bound clamped to [0, W] / [0, H]
 *   empty bin (y_hi <= y_lo or x_hi <= x_lo):  value 0, argmax -1
 *   else  v = -FLT_MAX, idx = -1;  y ascending, then x ascending:  if feat[b,y,x,c] > v then v = that pixel, idx = y * W + x
 * The strict > sends ties to the first pixel in row-major order and never selects NaN; a bin whose pixels are all -inf or
 * NaN yields -FLT_MAX with argmax -1.  argmax == NULL (inference) stores no indices.  The mask-cat forward writes
 * cat[..., :C] = v and cat[..., C:] = fl(v * masks[k,ph,pw]) in the same launch.
 *
 * Backward: grad_in[b, idx, c] += grad_out[k,ph,pw,c] for every argmax idx != -1 (mask-cat: += fl(dlo + fl(mask * dhi))), nothing
 * else; every element of grad_in is written (zero where nothing lands).  It takes rois and spatial_scale besides argmax: the
 * image of ROI k is rois[k][0], and the bins' bounds tell a workgroup which bins can reach its pixels.  argmax must be what the
 * forward wrote for these rois and this scale: an index outside its own bin's bounds is left out, never stored out of range.
 * No float atomics; per destination the terms are added in ascending (k, ph, pw) inside a group of ROIs and the groups in
 * order: two calls give the same bits.  scratch: cim_roi_pool_bwd_scratch(K,B,C,H,W,P) bytes for the groups' partial maps
 * (0: one group, scratch may be NULL), the caller's, 16-byte aligned for the 16-byte form of the sum; P does not enter today.
 *
 * Refused (-1, before any device work): a null pointer (except argmax in the forward, scratch where 0 bytes are asked for, and
 * the per-ROI arrays when K == 0), B, C, H, W or P below 1, K < 0, H W >= 2^31, K P P C (mask-cat: K P P 2C) >= 2^31.  K == 0
 * succeeds: the forward writes nothing, the backward an all-zero grad_in.  NOT checked: a batch index outside [0, B) is the
 * caller's error and no refusal - such a ROI comes out as a malformed one and receives no gradient.  Re-entrant: no state, caller's stream and scratch. */
int cim_roi_pool_fwd(const float* feat, const float* rois, float* out, int* argmax,
                     int B, int C, int H, int W, int K, int P, float spatial_scale, void* stream);
int cim_roi_pool_maskcat_fwd(const float* feat, const float* rois, const float* masks, float* cat, int* argmax,
                             int B, int C, int H, int W, int K, int P, float spatial_scale, void* stream);
long long cim_roi_pool_bwd_scratch(int K, int B, int C, int H, int W, int P);
int cim_roi_pool_bwd(const float* grad_out, const float* rois, const int* argmax, float* grad_in,
                     int B, int C, int H, int W, int K, int P, float spatial_scale, float* scratch, void* stream);
int cim_roi_pool_maskcat_bwd(const float* grad_cat, const float* rois, const float* masks, const int* argmax, float* grad_in,
                             int B, int C, int H, int W, int K, int P, float spatial_scale, float* scratch, void* stream);

/* ------------------------------------------------------------------ mask IoU / containment maps (a-7)
 * Replaces lib/utils/mask_utils.py:6-18 (mask_iou) and :20-32 (mask_asymmetric_iou) as driven
 * by tools/pre/create_cob_iou.py:43-49 / create_cob_asy_iou.py:43-53, and the per-step
 * pickle.load + H2D at lib/modeling/model_builder.py:147-159.
 *   iou[i,j] = |m_i & m_j| / |m_i | m_j|      asy[i,j] = |m_i & m_j| / |m_j|
 * with the reference's rounding chain int64 -> f64 divide -> f32 -> f16.
 */
/* masks_u8 [N, HW] (non-zero = inside) -> packed [words, N] uint64 (WORD-MAJOR: packed[w*N + n]),
 * words = ceil(HW/64), bit b of word w = pixel 64*w+b, tail bits zero. */
int cim_mask_pack(const uint8_t* masks_u8, uint64_t* packed, int N, int HW, void* stream);

/* packed [words,N] (word-major) -> area [N] int32, iou_f16 [N,N], asy_f16 [N,N]. */
int cim_mask_iou_pair(const uint64_t* packed, int N, int words, int32_t* area,
                      uint16_t* iou_f16, uint16_t* asy_f16, void* stream);

/* ------------------------------------------------------------------ CIM mining (a-4)
 * Replaces CIM_layer.CIM_label / MIST_label / instance_nms, lib/modeling/heads.py:237-407.
 * All index outputs are bit-identical to the reference CPU path.
 */
/* heads.py:338: flag[i] = (#{j : asy[i,j] > con_thr}) < 0.9*N     (flag: uint8 [N]) */
int cim_asy_flag(const uint16_t* asy_f16, int N, float con_thr, uint8_t* flag, void* stream);

/* Everything the mining needs from the containment map ALONE (an input of the step: the host runs this on a side stream under
 * the backbone forward): flags [n_slots, N] = cim_asy_flag for each of the n_slots distinct con_thr values (con_thr_host: HOST
 * array), and asy_t [N, ldt] = the map transposed, rows padded to ldt = 8 ceil(N / 8) entries (16-byte aligned rows, pad entries
 * zero; may be NULL) - the containment step reads whole COLUMNS of the map (heads.py:386: every proposal against one seed),
 * contiguous rows of the transposed copy. */
int cim_asy_prep(const uint16_t* asy_f16, int N, const float* con_thr_host, int n_slots, uint8_t* flags, uint16_t* asy_t,
                 void* stream);

/* The whole mining + assignment of ONE training step - all REFINE_TIMES CIM layers - without a host round trip:
 * 2 launches (seed selection + containment arg-max + arbitration + anti-noise sampling; assignment).
 * Replaces, per layer, CIM_layer.forward = CIM_label / MIST_label + instance_nms + the sampling loop + the assignment,
 * lib/modeling/heads.py:237-503, as called three times per image from lib/modeling/model_builder.py:170-187.
 *
 * The image's classes are read on the device: class c is active iff labels[c] != 0 (heads.py:340); per-class outputs
 * are indexed by the class id c itself.
 *
 * Per layer (cim_mining_layer):
 *   seed_score  top-K ranking score, element (i, c) at seed_score[i*seed_ld + seed_off + c]        (heads.py:354 / :279)
 *   det         containment arg-max score, element (i, c) at det[i*det_ld + det_off + c*det_cs]; det_cs = 0 selects the
 *               class-agnostic detector (heads.py:346-347); unused (may be NULL) when using_cim == 0 (MIST_label)
 *   wa, wb      arbitration weight (i, c) = wa[i*wa_ld + wa_off + c] * (wb ? wb[i*wb_ld + wb_off + c*wb_cs] : 1)
 *               (preds = cls * det, heads.py:330,397; MIST: the product tensor itself, wb = NULL, :306)
 *   nms_thr, cls_thr, iou_thr, con_thr   Python-float thresholds (rounded to binary16 inside)
 *   using_cim   1: CIM_label (seeds -> containing proposals), 0: MIST_label (seeds are the pseudo GTs)
 *   anti_noise  1: resample each class's pseudo GTs in proportion to their weight (heads.py:447-473)
 *   flag_slot   which of the `flags` arrays (one per distinct con_thr, written by cim_asy_flag beforehand) this layer uses
 * Outputs per layer:
 *   topk [C,K] i32 (keep_sort_idx), seeds [C,K] i32 (keep_nms_idx in selection order, -1 beyond n_seeds[c]),
 *   n_seeds [C] i32, res [C,K] i32 (res_idx per seed, -1: no containing proposal / no seed; CIM layers only)
 *   gt_class [N] i32 (0 / class id + 1), gt_weight [N] f32 (-1 where unset)             after arbitration
 *   pre_idx [N] i32, pre_keep [N] u8: the G pseudo GTs in ascending proposal order and the sampling keep-mask over them
 *   gt_idx [N] i32, gt_cls [N] i32, gt_w [N] f32: the G' survivors;  counts [2] i32 = { G, G' }
 *   pseudo_labels [N,C+1] f32, pseudo_iou [N] binary16 {0,1}, loss_weights [N] f32, max_idx [N] i32   (heads.py:477-501;
 *   NOT written when G == 0: the reference returns (None, None, None) and the model skips the layer, :429-430)
 * Step-wide:
 *   flags [n_slots, N] u8 (cim_asy_flag), uniforms [max_uniforms] f64 = the next doubles of the host's MT19937 stream
 *   (np.random.random_sample), consumed in the order of the reference's sequential calls; used [1] i32 = how many were
 *   consumed; layer_valid [R] i32 = (G > 0); status [1] i32 error bits (0 = ok; 1: class list longer than K, 2: uniforms
 *   exhausted; the losses launch ORs 4 / 8 into it, see cim_loss_args).
 * Limits: N <= 8192, K <= 1024, R <= CIM_MAX_LAYERS. */
#define CIM_MAX_LAYERS 4
typedef struct cim_mining_layer {
    const float* seed_score; int32_t seed_ld, seed_off;
    const float* det;        int32_t det_ld, det_off, det_cs;
    const float* wa;         int32_t wa_ld, wa_off;
    const float* wb;         int32_t wb_ld, wb_off, wb_cs;
    float nms_thr, cls_thr, iou_thr, con_thr;
    int32_t using_cim, anti_noise, flag_slot, reserved_;
    int32_t* topk; int32_t* seeds; int32_t* n_seeds; int32_t* res;
    int32_t* gt_class; float* gt_weight;
    int32_t* pre_idx; uint8_t* pre_keep;
    int32_t* gt_idx; int32_t* gt_cls; float* gt_w; int32_t* counts;
    float* pseudo_labels; uint16_t* pseudo_iou; float* loss_weights; int32_t* max_idx;
} cim_mining_layer;

typedef struct cim_mining_args {
    int32_t N, C, K, R;
    const float* labels;             /* [C] image labels */
    const uint16_t* iou;             /* [N,N] binary16 mask-IoU map */
    const uint16_t* asy;             /* [N,N] binary16 containment map */
    const uint16_t* asy_t;           /* [N, 8 ceil(N/8)] its transpose from cim_asy_prep (NULL: the map's columns are read with strided loads) */
    const uint8_t* flags;            /* [n_slots, N] from cim_asy_flag */
    const double* uniforms;          /* [max_uniforms] */
    int32_t max_uniforms, reserved_;
    int32_t* used;                   /* [1] */
    int32_t* status;                 /* [1] */
    int32_t* layer_valid;            /* [R] */
    cim_mining_layer layer[CIM_MAX_LAYERS];
} cim_mining_args;

/* Dynamic LDS of the mining launch (must be <= 156 KiB).
 * sync: cim_mining_sync_bytes() bytes of caller-owned device scratch, 8-byte aligned, ZERO-FILLED ONCE by the caller when it
 * is allocated: the workgroups of the mining launch meet through it (arrival counters of the (class, layer) workgroups - a
 * layer's last arrival runs its arbitration -, the list lengths the layers hand each other for the position in the uniform
 * stream) and the call leaves every word zero again, so the same scratch serves the next call on that stream and the launches
 * can be captured into a HIP graph.  Calls that may be in flight TOGETHER (two streams) need a scratch each. */
long long cim_mining_lds_bytes(int N, int K);
/* Which form of the seed phase a call with these sizes runs (host only, additive: cim_abi_version() stays 16): bit 0 = the
 * layer's detector column and flags are staged in LDS, bit 1 = the NMS bit-matrix comes from whole map rows streamed through LDS
 * (else from K x K single gathers).  0 for N <= 0 or K <= 0. */
long long cim_mining_layout(int N, int K);
long long cim_mining_sync_bytes(void);
int cim_mining_step(const cim_mining_args* args, void* sync, void* stream);

/* ------------------------------------------------------------------ detection post-processing (inference's last stage)
 * Replaces box_results_with_nms_and_limit / box_results_for_corloc (lib/core/test.py:320-420) and
 * mask_results_with_nms_and_limit{,_get_index} (lib/utils/mask_eval_utils.py:6-108): per class, the proposals with
 * scores[p, c] > score_thr, greedy box NMS at nms_thr (lib/utils/cython_nms.pyx:36-87), then the per-image limit over ALL
 * classes: when more than max_det boxes are kept (max_det > 0), only those whose score is >= the max_det-th largest kept
 * score stay (ties at that score all stay, so more than max_det can remain).
 *
 * scores [N, ld] f32 (row p, column c; ld >= C), boxes [N, 4] f32 (x1, y1, x2, y2; 16-byte aligned),
 * 1 <= N <= CIM_DETECT_MAX_N, C >= 1; other shapes are refused before any launch (-1).  ws: cim_detect_ws_bytes(N, C)
 * bytes, 8-byte aligned, no initial content.  Outputs:
 *   det [C * N][3] i32   records (proposal, class, score bit pattern) in (class ascending, proposal ascending) order -
 *                        what the reference's keep lists hold (keep comes back in ascending proposal order, not by score);
 *                        the first *total are written
 *   count_per_class [C]  records per class;  total [1]: records in all
 * Exactness: the overlap is the pyx's fp32 arithmetic operation for operation (no contraction, correctly rounded
 * division, its >= / <= ternaries for max / min), compared as ovr >= nms_thr; scores compare as s > score_thr in fp32.
 * Tie rule: candidates of equal score are visited HIGHER proposal index first (np.argsort(s, kind="stable")[::-1]; the
 * reference's unstable default sort leaves this order undefined).
 * Three launches (overlap matrix, one workgroup per class, one limit workgroup); no host synchronisation. */
#define CIM_DETECT_MAX_N 8192
long long cim_detect_ws_bytes(int N, int C);
int cim_detect_nms_limit(const float* scores, int ld, const float* boxes, int N, int C, float score_thr, float nms_thr,
                         int max_det, void* ws, int32_t* det, int32_t* count_per_class, int32_t* total, void* stream);
/* CorLoc (lib/core/test.py:320-352): per class, np.argmax(scores[:, c]) - the first index of the maximum, the first NaN if
 * any.  out [C][2] i32 = (proposal, score bit pattern).  Same shape limits as above. */
int cim_detect_corloc(const float* scores, int ld, int N, int C, int32_t* out, void* stream);

/* Ragged batch form (additive: cim_abi_version() stays 16): the same stage for B images in ONE call of five
 * launches - a one-workgroup prologue (per-image words and offsets from row_off), the 64 x 64 overlap tiles of all images in
 * a 1-D grid, the NMS on a (C, B) grid, one limit workgroup per image, and the compaction of the records.  Each per-image
 * body is the device code of the single-image entry above, so its exactness contract and tie rule hold unchanged.
 *
 * scores [sum N, ld] f32 and boxes [sum N, 4] f32, the images back to back; row_off [B + 1] i32 (image b = rows
 * row_off[b] .. row_off[b + 1]) twice: on the device (what the kernels read) and on the host (sizes the grids and the
 * workspace, validates the shapes; the launches do nothing and total[b] = -1 if the two disagree).  One score_thr, nms_thr
 * and max_det for the call.  Limits, refused before any launch (-1, cim_last_error() names them): 1 <= B <=
 * CIM_BATCH_DETECT_MAX_IMAGES, row_off[0] = 0, every 1 <= N_b <= CIM_DETECT_MAX_N, C >= 1, 3 * C * sum N < 2^31, ld >= C.
 *   area_bounds [B][2] f32 = (lo_b, hi_b) on the device, or NULL: TEST.PROPOSAL_FILTER (tools/evaluation.py:108-115) - a
 *       proposal whose (x2 - x1) * (y2 - y1) (fp32, no + 1) is > hi_b or < lo_b has its score read as 0.0f for every class,
 *       before the s > score_thr test; both compares are strict.  Needs score_thr >= 0 (a zero score is then no candidate).
 *   class_mask [B][C] u8 on the device, or NULL: only classes with a nonzero entry are written - applied AFTER the limit
 *       over all classes (tools/generate_mask_for_MaskRCNN.py:124-136), never before.
 *   ws: cim_batch_detect_ws_bytes(row_off (host), B, C) bytes, 8-byte aligned, no initial content.
 * Outputs: det [C * sum N][3] i32 records (proposal WITHIN its image, class, score bit pattern) of all images in one
 * contiguous array, in (image, class ascending, proposal ascending) order - the first sum(total) are written;
 * count [B][C] records per (image, class); total [B] records per image.  No allocation, no host copy, no synchronisation. */
#define CIM_BATCH_DETECT_MAX_IMAGES 4096
long long cim_batch_detect_ws_bytes(const int32_t* row_off_host, int B, int C);
int cim_batch_detect_nms_limit(const float* scores, int ld, const float* boxes, const int32_t* row_off_dev,
                               const int32_t* row_off_host, int B, int C, float score_thr, float nms_thr, int max_det,
                               const float* area_bounds, const unsigned char* class_mask, void* ws, int32_t* det,
                               int32_t* count, int32_t* total, void* stream);

/* Soft-NMS and box voting (additive: cim_abi_version() stays 16): TEST.SOFT_NMS / TEST.BBOX_VOTE of
 * box_results_with_nms_and_limit (lib/core/test.py:378-396) - cython_nms.pyx:98-203 (soft_nms), boxes.py:268-317
 * (box_voting) over cython_bbox.pyx:32-73 (bbox_overlaps) - followed by the same per-image limit.  Same inputs, shape limits
 * and refusals as cim_detect_nms_limit.
 *   nms_kind   CIM_SOFTVOTE_NMS_GREEDY: the greedy pass of cim_detect_nms_limit (its bits, its tie rule).  SOFT_HARD / LINEAR /
 *              GAUSSIAN: per class, on the candidates s > score_thr in ascending proposal order, the pyx's loop - select the
 *              FIRST position of the maximum score, swap it forward, decay every later row that overlaps it (iw > 0 and ih > 0)
 *              by the method's weight (overlap threshold nms_thr, gaussian: (float)exp((double)(-(ov * ov) / sigma))), drop a
 *              decayed row whose score is < soft_min_score by overwriting it with the last row.  A row that overlaps nothing is
 *              never dropped.  Records come in SELECTION order with the DECAYED scores, bit for bit the pyx's (fp32 operation
 *              for operation, ties by array position), given finite boxes and a device exp() that rounds to the same fp32.
 *   vote       nonzero: every record's box becomes the score-weighted mean of the class's candidates whose fp32 overlap with
 *              it is >= vote_thr, and its score follows scoring_method (CIM_SOFTVOTE_SCORE_*, beta as in boxes.py); sums are
 *              taken in double in a fixed order (the same bits on every run and stream).  Needs score_thr >= 0 (weights > 0).
 *              A record with no voter gets NaN and adds 1 to *empty_votes (the reference raises ZeroDivisionError there).
 *   max_det    the limit over all classes AFTER soft-NMS / voting, on the decayed / re-scored values; record order is kept.
 *   ws         cim_softvote_ws_bytes(N, C) bytes, 16-byte aligned, no initial content.
 * Outputs: det [C * N][3] i32 records (proposal, class, score bit pattern), class ascending, within a class the order above;
 * det_boxes [C * N][4] f32 (16-byte aligned) the records' boxes - voted, or the proposals' -; count_per_class [C]; total [1];
 * empty_votes [1].  One memset and 3 - 5 launches, no host synchronisation. */
#define CIM_SOFTVOTE_NMS_GREEDY 0
#define CIM_SOFTVOTE_NMS_SOFT_HARD 1
#define CIM_SOFTVOTE_NMS_SOFT_LINEAR 2
#define CIM_SOFTVOTE_NMS_SOFT_GAUSSIAN 3
#define CIM_SOFTVOTE_SCORE_ID 0
#define CIM_SOFTVOTE_SCORE_AVG 1
#define CIM_SOFTVOTE_SCORE_IOU_AVG 2
#define CIM_SOFTVOTE_SCORE_QUASI_SUM 3
#define CIM_SOFTVOTE_SCORE_GENERALIZED_AVG 4
#define CIM_SOFTVOTE_SCORE_TEMP_AVG 5
long long cim_softvote_ws_bytes(int N, int C);
int cim_softvote_postprocess(const float* scores, int ld, const float* boxes, int N, int C, float score_thr, float nms_thr,
                             int nms_kind, float sigma, float soft_min_score, int vote, float vote_thr, int scoring_method,
                             float beta, int max_det, void* ws, int32_t* det, float* det_boxes, int32_t* count_per_class,
                             int32_t* total, int32_t* empty_votes, void* stream);
/* box_voting on arbitrary top boxes: all_boxes [K][4] and all_scores [K] vote (every row, scores as weights) for top_boxes
 * [T][4]; out_boxes [T][4] the voted boxes, out_scores [T] the scores by scoring_method (left untouched for ID), empty_votes
 * [1] as above.  K >= 1, T >= 1; the box arrays 16-byte aligned.  One memset and one launch. */
int cim_softvote_vote(const float* all_boxes, const float* all_scores, int K, const float* top_boxes, int T, float vote_thr,
                      int scoring_method, float beta, float* out_boxes, float* out_scores, int32_t* empty_votes,
                      void* stream);

/* ------------------------------------------------------------------ instance-segmentation evaluation (ABI-16 addition)
 * Replaces pycocotools' mask.encode / decode / iou and COCOeval(..., 'segm').evaluateImg / accumulate as the reference runs
 * them (tools/evaluation.py:72-145, 236-241; lib/datasets/json_inference.py:24-55; lib/utils/mask_eval_utils.py:113-116).
 * Additive: cim_abi_version() stays 16.  Exactness contract and limits: DESIGN.md 4.12.
 *
 * Packed masks: uint64 [n][words], words = cim_segm_words(H, W) = ceil(H W / 64), pixel (y, x) at column-major position
 * p = x H + y = bit p & 63 of word p >> 6; bits past H W are 0.
 *   cim_segm_pack        [n_src, H, W] uint8 / bool masks (row-major, nonzero = 1) -> packed; idx [n] int64 (may be NULL =
 *                        0..n-1) picks the source masks (an index outside [0, n_src) packs an empty mask)
 *   cim_segm_area        pixel count per packed mask
 *   cim_segm_rle_count   len [n] = number of COCO run counts per mask (column-major runs, alternating, starting with a
 *                        zero-run, possibly empty: pycocotools' rleEncode)
 *   cim_segm_rle_write   the counts (uint32) of mask i at counts[off[i] ...], len[i] of them (from cim_segm_rle_count)
 *   cim_segm_rle_decode  counts -> packed masks; ws: cim_segm_rle_decode_ws_bytes(sum of len) bytes.  Pixels past the sum
 *                        of a mask's counts stay 0, counts past H W are clipped.
 * Per image (cim_segm_eval_image): detections in (image, category) groups, each sorted by -score (stable over the input
 * order) and cut to its nd = min(n, maxDets[-1]); IoU inter / (area_d + area_g - inter) (inter / area_d for a crowd ground
 * truth; 0 when inter == 0) in fp64 from integer popcounts; then evaluateImg's greedy matching per (group, area range,
 * threshold).  meta int32: groups [n_groups][8] = (det_start, n_det, gt_start, n_gt, nd, rec_off, pair_off, 0) -
 * det_start / gt_start index det_list / gt_list, rec_off is the group's byte offset in `records`
 * (cim_segm_record_bytes(nd, n_gt, A, T) bytes, 8-byte aligned), pair_off its first entry of the nd x n_gt IoU block
 * (pairs in all); then det_list [n_dl] (image detection indices, input order), gt_list [n_gl] (image ground-truth indices,
 * input order), crowd [G].  gt_area [G] f64 is the annotations' `area`, gt_id [G] int64 their ids, iou_thrs [T] and
 * area_rng [A][2] f64 the host's values.  ws: cim_segm_image_ws_bytes(D, G, pairs) bytes.  A record holds, in rank order:
 * dtm int64 [A][T][nd] (matched ground-truth id, 0 = none), score f32 [nd], order int32 [nd], npig int32 [A], gt_order
 * int32 [A][n_gt], dt_ignore uint8 [A][T][nd], gt_ignore uint8 [A][n_gt] (layout: csrc/eval_match.h rec_layout).
 * Accumulate (cim_segm_accumulate): entries [n_entries][6] int64 = (record device address, nd, n_gt, first element,
 * category index, 0), category-major and image-minor (ascending image id), one per (image, category) with a ground truth
 * or a detection; cat_off [K + 1] the first element of each category (E elements in all); jobs [.][3] int64 = (start,
 * lenA, lenB) of the bottom-up merge rounds of the per-image runs, round r's jobs at round_off[r] .. round_off[r + 1];
 * rec_thrs [R] f64, max_dets [M] int32 (ascending).  Outputs (f64): precision / scores [T][R][K][A][M], recall
 * [T][K][A][M], -1 where COCOeval leaves -1.  ws: cim_segm_accumulate_ws_bytes(E, K, A, T) bytes. */
#define CIM_SEGM_MAX_HW (1 << 22)       /* pixels per mask */
#define CIM_SEGM_MAX_GT 1024            /* ground truths per image */
#define CIM_SEGM_MAX_T 16               /* IoU thresholds */
#define CIM_SEGM_MAX_R 128              /* recall thresholds */
#define CIM_SEGM_MAX_A 8                /* area ranges */
#define CIM_SEGM_MAX_M 4                /* maxDets */
/* detections per (image, category) and maxDets[-1]: <= CIM_DETECT_MAX_N */
int cim_segm_words(int H, int W);
int cim_segm_pack(const uint8_t* masks, const int64_t* idx, long long n_src, int n, int H, int W, uint64_t* packed, void* stream);
int cim_segm_area(const uint64_t* packed, int n, int words, int32_t* area, void* stream);
int cim_segm_rle_count(const uint64_t* packed, int n, int H, int W, int32_t* len, void* stream);
int cim_segm_rle_write(const uint64_t* packed, int n, int H, int W, const int64_t* off, const int32_t* len, uint32_t* counts,
                       void* stream);
long long cim_segm_rle_decode_ws_bytes(long long total_counts);
int cim_segm_rle_decode(const uint32_t* counts, const int64_t* off, const int32_t* len, int n, int H, int W, void* ws,
                        uint64_t* packed, void* stream);
long long cim_segm_image_ws_bytes(int D, int G, long long pairs);
long long cim_segm_record_bytes(int nd, int ng, int A, int T);
int cim_segm_eval_image(const uint64_t* dt_packed, int D, const uint64_t* gt_packed, int G, int words, const float* dt_score,
                        const int32_t* meta, int n_groups, int n_dl, int n_gl, long long pairs, const double* gt_area,
                        const int64_t* gt_id, const double* iou_thrs, int T, const double* area_rng, int A, void* ws,
                        void* records, void* stream);
long long cim_segm_accumulate_ws_bytes(long long E, int K, int A, int T);
int cim_segm_accumulate(const int64_t* entries, int n_entries, long long E, int K, const int64_t* cat_off, const int64_t* jobs,
                        const int64_t* round_off, int rounds, const double* rec_thrs, int R, const int32_t* max_dets, int M,
                        int A, int T, void* ws, double* precision, double* recall, double* scores, void* stream);

/* ------------------------------------------------------------------ polygon ground truth for mask AP (ABI-16 addition)
 * COCO's polygon fill (maskApi.c rleFrPoly, then merge as a union): what pycocotools' annToRLE / frPyObjects does to an
 * annotation whose `segmentation` is a list of polygons, straight to the packed masks above (csrc/poly_fill.hip).
 * Additive: cim_abi_version() stays 16.  Exactness contract (bit-identical to tests/golden/poly_np.py): DESIGN.md 4.12.
 *
 * cim_poly_fill, all pointers device memory:
 *   xy [2 n_vert] f64       the polygons' coordinates x0, y0, x1, y1, ... back to back (each finite, within [-2^20, 2^20])
 *   poly_off [n_poly + 1]   int32 first vertex of each polygon (ascending, poly_off[n_poly] = n_vert, >= 3 vertices each)
 *   poly_ann [n_poly]       int32 annotation (row of `packed`) each polygon belongs to; a value outside 0..n_ann-1 is skipped
 *   edge_off [n_vert + 1]   int32 exclusive prefix of the edges' dense-point counts: edge j runs from vertex j to the next
 *                           vertex of its polygon (the last one back to the first) and has max(|dX|, |dY|) + 1 points, X =
 *                           (int)(5 x + .5), Y likewise; edge_off[n_vert] = n_points
 *   packed [n_ann][words]   uint64 out, words = cim_segm_words(H, W): the OR of each annotation's polygon fills, bits past
 *                           H W zero, an annotation without polygons empty
 * ws: cim_poly_ws_bytes(n_poly, H, W) bytes, 8-byte aligned, no initial content; one ws serves one call at a time.
 * Two memsets and two launches on `stream` (crossings: one lane per dense point; fill: one workgroup per polygon); no host
 * synchronisation.  Refused before any launch (-1): H W > CIM_SEGM_MAX_HW, n_points > CIM_POLY_MAX_POINTS (2^26: one lane
 * per point keeps the crossing launch at <= 2^18 workgroups and every offset in int32), counts that cannot fit together.
 * The coordinates are the caller's to check (cim_amd.segm_eval.poly_masks refuses odd lengths, fewer than 6 numbers,
 * non-finite values and values outside [-2^20, 2^20]); whatever the arrays hold, nothing is read or written out of range. */
#define CIM_POLY_MAX_POINTS (1 << 26)   /* dense points per call */
long long cim_poly_ws_bytes(int n_poly, int H, int W);
int cim_poly_fill(const double* xy, const int32_t* poly_off, const int32_t* poly_ann, const int32_t* edge_off, int n_poly,
                  int n_vert, long long n_points, int n_ann, int H, int W, void* ws, uint64_t* packed, void* stream);

/* ------------------------------------------------------------------ box evaluation (ABI-16 addition)
 * Scores the boxes inference produced, as the reference's task_evaluation.evaluate_all does: COCOeval(..., 'bbox')
 * (lib/datasets/json_dataset_evaluator.py:105-118), the VOC devkit's AP (lib/datasets/voc_eval.py:146-228) and CorLoc
 * (lib/datasets/dis_eval.py:88-141); csrc/box_eval.hip.  Additive: cim_abi_version() stays 16.  Exactness contract, limits
 * and the tie rule: DESIGN.md 4.14.  All box arithmetic is fp64, every operation rounded on its own (no contraction).
 *
 * cim_box_eval_image: cim_segm_eval_image with boxes in place of packed masks - the same meta, records, gt_area, gt_id,
 * iou_thrs and area_rng, the same record layout (cim_segm_record_bytes), so cim_segm_accumulate consumes the records
 * unchanged.  dt_box [D][4], gt_box [G][4] f64 = (x, y, w, h).  IoU: maskApi.c's bbIou operation for operation - da =
 * D[2] D[3], ga = G[2] G[3], w = fmin(D[2] + D[0], G[2] + G[0]) - fmax(D[0], G[0]), h likewise on y, 0 when w <= 0 or
 * h <= 0, else i = w h and i / (crowd ? da : da + ga - i).  A detection's area for the area-range rule is da (what
 * COCO.loadRes stores for a bbox result), not a pixel count.  ws: cim_box_image_ws_bytes(D, G, pairs) bytes, 8-byte aligned.
 * Four launches (areas, sort, IoU, match - the matcher is cim_segm_eval_image's own, csrc/eval_match.h).
 *
 * cim_voc_match: the whole dataset in one launch, one workgroup per (class, image) group.  groups [n_groups][4] int32 =
 * (det_start, n_det, gt_start, n_gt) into dt_box [D][4] / dt_conf [D] f64 and gt_box [G][4] f64 / gt_difficult [G] uint8,
 * boxes as (x1, y1, x2, y2); n_det <= CIM_DETECT_MAX_N and n_gt <= CIM_SEGM_MAX_GT per group (more are not visited; a group
 * that does not lie inside the arrays is left alone).  Within a group detections are visited by descending confidence,
 * equal confidences in ascending input position (a stated deviation: the reference's np.argsort(-confidence) leaves ties
 * undefined).  Per detection voc_eval's arithmetic (the + 1 widths, inters / uni), ovmax = the maximum overlap, jmax = its
 * first index; with ovmax > ovthresh a difficult ground truth gives neither tp nor fp, an unclaimed one tp (and is claimed),
 * a claimed one fp; otherwise, and with n_gt = 0, fp.  mode 1 is dis_eval's rule: tp if and only if ovmax > ovthresh (no
 * claims, no difficult flags), fp = 1 - tp.  Outputs by input position: tp, fp [D] uint8, ovmax [D] f64 (-inf without
 * ground truth), jmax [D] int32 (-1 without ground truth).
 *
 * cim_voc_ap: per class, voc_eval.py:219-226 and its voc_ap.  Detections class-major, class k at class_off[k] ..
 * class_off[k + 1] (int64 [K + 1]); npos [K] f64.  The stable sort by descending confidence over the input order is a rank
 * sort of each of runs [n_runs][2] int64 = (start, length <= CIM_VOC_MAX_RUN) - the runs tile [0, D) and none crosses a
 * class - followed by the bottom-up merge rounds of cim_segm_accumulate (jobs, round_off, rounds: the same arrays, over the
 * runs).  Then cumulative tp / fp, rec = tp / npos, prec = tp / max(tp + fp, DBL_EPSILON), written in sorted order at the
 * class's offsets, and ap [K]: with thr11 != NULL the 11-point form over the host's 11 fp64 thresholds (ap = ap + p / 11. in
 * their order), with thr11 == NULL the area form (precision envelope from the right, the sum of (mrec[i + 1] - mrec[i])
 * mpre[i + 1] where recall changes; the sum's order differs from NumPy's pairwise one).  A class without
 * detections: ap = 0; npos = 0: IEEE division (NaN recall: ap = 0 in the 11-point form, NaN in the area form).
 * ws: cim_voc_ap_ws_bytes(D) bytes, 8-byte aligned.  One memset and 2 + rounds launches.
 * None of the three allocates, synchronises or keeps state.  Whatever the box, confidence, flag, group, run and class_off
 * arrays hold, nothing is read or written out of range; round_off and jobs are trusted as an index structure (round_off
 * ascending within the jobs array, as cim_segm_accumulate trusts them), while a job that does not lie inside [0, D) moves nothing. */
#define CIM_VOC_MAX_RUN 256             /* detections per run of cim_voc_ap */
long long cim_box_image_ws_bytes(int D, int G, long long pairs);
int cim_box_eval_image(const double* dt_box, int D, const double* gt_box, int G, const float* dt_score, const int32_t* meta,
                       int n_groups, int n_dl, int n_gl, long long pairs, const double* gt_area, const int64_t* gt_id,
                       const double* iou_thrs, int T, const double* area_rng, int A, void* ws, void* records, void* stream);
int cim_voc_match(const double* dt_box, const double* dt_conf, int D, const double* gt_box, const uint8_t* gt_difficult, int G,
                  const int32_t* groups, int n_groups, double ovthresh, int mode, uint8_t* tp, uint8_t* fp, double* ovmax,
                  int32_t* jmax, void* stream);
long long cim_voc_ap_ws_bytes(long long D);
int cim_voc_ap(const double* dt_conf, const uint8_t* tp, const uint8_t* fp, long long D, const int64_t* class_off,
               const double* npos, int K, const int64_t* runs, int n_runs, const int64_t* jobs, const int64_t* round_off,
               int rounds, const double* thr11, void* ws, double* rec, double* prec, double* ap, void* stream);

/* ------------------------------------------------------------------ training inputs from proposal masks (ABI-16 addition)
 * Replaces tools/pre/generate_7_7_{voc,coco}.py:35-42 (tight boxes, PIL nearest resize to S x S) and the label assignment of
 * tools/pre/AGPL_label_assign.py:154-180 / point_level_label_assign.py:66-93 (lib/utils/mask_utils.py:6-18).
 * Additive: cim_abi_version() stays 16.  Exactness contract and limits: DESIGN.md 4.13.
 *
 * Shapes refused before any launch (-1): N < 1, H or W outside 1..65535 (the reference stores boxes as uint16),
 * H W > CIM_SEGM_MAX_HW, S outside 1..CIM_PROP_MAX_S, P outside 0..CIM_PROP_MAX_POINTS, a class outside 0..C-1, a point
 * outside the image (NumPy would wrap a negative index: a stated deviation).
 * ws: cim_prop_ws_bytes(N, H W, P) bytes (P = 0 for the prepare call alone), 8-byte aligned, no initial content; one ws serves
 * one call at a time.
 *
 * cim_prop_prepare: masks_u8 [N, H W] (non-zero = inside; pixel (y, x) at y W + x) ->
 *   packed [words, N] uint64   exactly what cim_mask_pack writes (it is the one launch that reads masks_u8),
 *   boxes [N, 4] int32         (xmin, ymin, xmax + 1, ymax + 1) of the set pixels,
 *   area [N] int32, small [N, S, S] uint8 (0 / 1): the crop to the box resized as PIL's nearest filter does,
 *   empty_flag [1] int32       0, or N - n for the first proposal n without a set pixel (its box, area and small are 0; the
 *                              reference raises there, so nothing else is defined for such an image).
 * Three launches (pack, extents from the words, resize); no host synchronisation.
 *
 * cim_prop_assign: packed / area as above; rows, cols, classes [P] int32 are HOST arrays, read before the call returns (the
 * points travel in the kernel arguments), in the order the reference visits them; mat [N, C + 1] f32 out: at most one
 * non-zero per row, the cluster number j + 1 of the LAST point j whose average mask the proposal overlaps by IoU > 0.5 in
 * column class_j + 1, else P + 1 in column 0 when 0 < IoU <= 0.5 for some point; every row (1, 0, ...) when P = 0.
 * Three launches (average masks, intersections, the sequential rule); no host synchronisation. */
#define CIM_PROP_MAX_POINTS 256
#define CIM_PROP_MAX_S 16
long long cim_prop_ws_bytes(int N, int HW, int P);
int cim_prop_prepare(const uint8_t* masks_u8, int N, int H, int W, int S, uint64_t* packed, int32_t* boxes, int32_t* area,
                     uint8_t* small, int32_t* empty_flag, void* ws, void* stream);
int cim_prop_assign(const uint64_t* packed, const int32_t* area, int N, int H, int W, const int32_t* rows, const int32_t* cols,
                    const int32_t* classes, int P, int C, float* mat, void* ws, void* stream);

/* ------------------------------------------------------------------ PRM peaks: class response maps to cluster points (ABI-16 addition)
 * Replaces what tools/pre/AGPL_label_assign.py:136-161 reads from lib/prm/prm_model_gt.py:216-310 (PeakResponseMapping.forward
 * in inference mode) and lib/prm/prm_modules.py:9-44 (PeakStimulation): the bilinear sub-pixel up-sampling of the class response
 * maps, the median-filtered 3 x 3 peak test, the threshold / fallback selection and the ascending-score order, for a BATCH of
 * images and only for the (image, class) PAIRS the caller names.  The peak back-propagation (the peak response maps) is not
 * computed: the label assignment reads only their number.  Additive: cim_abi_version() stays 16.  Exactness contract: DESIGN.md 4.19.
 *
 * desc: int32 [2 M + 2 B] = pair image [M] | pair class [M] | image height [B] | image width [B]; the caller passes it twice,
 * desc_host (HOST memory, read and checked before the call returns) and desc_dev (the same words in device memory, read by the
 * kernels).  The pairs of an image are contiguous, images ascending, classes in the caller's order (the order of `lables`).
 * Refused before any launch (-1, cim_last_error() names the condition): M < 1, B < 1, H W > CIM_PRM_MAX_HW, factor < 1, a class
 * outside 0..C-1, an image index outside 0..B-1 or smaller than its predecessor, an image side outside 1..65535.
 * ws: cim_prm_ws_bytes(M, HW) bytes, 8-byte aligned, no initial content, HW = 0 for cim_prm_peaks (which is given `up`).
 *
 * cim_prm_upsample: crm [B, C, h, w] f32 (+ bias [C] or NULL, added to every tap) -> up [M, factor h, factor w]: bilinear,
 *   align_corners = True, the arithmetic of DESIGN.md 4.19 (bit-identical to tests/golden/prm_np.py: upsample).  One launch.
 * cim_prm_peaks: up [M, H, W] f32 ->
 *   median [M] f32           the LOWER median of each map (torch.median: element (H W - 1) / 2 of the ascending order),
 *   pair_counts [M, 3] int32 all peaks (3 x 3 window, -inf padding, first maximum wins, value >= median) | valid peaks (value >
 *                            peak_threshold; 1 when none is and the fallback - the first peak holding the largest peak value -
 *                            stands in) | flags: CIM_PRM_STATUS_NAN, CIM_PRM_STATUS_NO_PEAK (a map of -inf only),
 *   per image b: image_out [B, 2] int32 = number of valid peaks (the TRUE number, also beyond CIM_PRM_MAX_PEAKS) | status (0, or
 *     CIM_PRM_STATUS_* bits; nothing else is written for an image whose status is not 0),
 *     points [B, CIM_PRM_MAX_PEAKS, 5] int32 = (row, col, class, y, x) in ascending score order, STABLE (equal scores keep the
 *     order pairs-then-row-major), row = y img_h / H, col = x img_w / W (integer division), scores [B, CIM_PRM_MAX_PEAKS] f32.
 *   Two launches (one workgroup per pair, one per image); no host synchronisation, no atomics deciding an order.
 * cim_prm_points: cim_prm_upsample into ws, then cim_prm_peaks on it: three launches. */
#define CIM_PRM_MAX_HW (1 << 22)
#define CIM_PRM_MAX_PEAKS (CIM_PROP_MAX_POINTS)   /* cim_prop_assign takes no more */
#define CIM_PRM_STATUS_TOO_MANY 1
#define CIM_PRM_STATUS_NAN 2
#define CIM_PRM_STATUS_NO_PEAK 4
long long cim_prm_ws_bytes(int M, int HW);
int cim_prm_upsample(const float* crm, const float* bias, int B, int C, int h, int w, int factor, int M, const int32_t* desc_host,
                     const int32_t* desc_dev, float* up, void* stream);
int cim_prm_peaks(const float* up, int M, int H, int W, int B, int C, const int32_t* desc_host, const int32_t* desc_dev,
                  float peak_threshold, float* median, int32_t* pair_counts, int32_t* points, float* scores, int32_t* image_out,
                  void* ws, void* stream);
int cim_prm_points(const float* crm, const float* bias, int B, int C, int h, int w, int factor, int M, const int32_t* desc_host,
                   const int32_t* desc_dev, float peak_threshold, float* median, int32_t* pair_counts, int32_t* points,
                   float* scores, int32_t* image_out, void* ws, void* stream);

/* ------------------------------------------------------------------ PRM classification training head: peak stimulation and loss (ABI-16 addition)
 * Replaces, for training the PRM classifier, what lib/prm/prm_model.py composes from F.upsample(align_corners=True), the
 * median filter, lib/prm/prm_modules.py:9-51 (PeakStimulation forward and backward) and F.multilabel_soft_margin_loss: class
 * response maps -> aggregated class scores -> loss, with the gradient back to the class response maps.  ALL B C maps are
 * processed, one 256-thread workgroup each; the up-sampled map lives in LDS and is never written to memory.  Stateless and
 * re-entrant on the caller's stream; no workspace; no float atomics; every sum in a fixed order.  Additive: cim_abi_version()
 * stays 16.  Exactness contract, the summation orders and the stated differences from the reference: DESIGN.md 4.21.
 * (The entries are named cim_prmt_*: "PRM training".)
 *
 * Refused before any launch (-1, cim_last_error() names the condition): B < 1, C < 1, h < 1, w < 1, factor < 1, an up-sampled
 * map of more than CIM_PRM_STIM_MAX_HW pixels (factor h x factor w; it has to fit LDS twice per CU), B C beyond 2^24, a NULL
 * pointer other than bias / dbias.
 *
 * cim_prmt_stim_forward: crm [B, C, h, w] f32 (+ bias [C] or NULL, added to every tap) -> per map, with H = factor h, W = factor w:
 *   the up-sampled map (the arithmetic of cim_prm_upsample, bit for bit), its LOWER median, the peak test of cim_prm_peaks
 *   (3 x 3 window, -inf padding, first maximum wins, value >= median),
 *   bitmap [B, C, ceil(H W / 32)] uint32: bit (p & 31) of word p >> 5 is set for a peak at pixel p = y W + x (nothing is dropped),
 *   count [B, C] int32 the number of peaks, median [B, C] f32,
 *   agg [B, C] f32 = (sum of the peak values, in the order of DESIGN.md 4.21) / count,
 *   status [B, C] int32 = 0, CIM_PRM_STATUS_NAN (a NaN in the up-sampled map) or CIM_PRM_STATUS_NO_PEAK (an up-sampled map of
 *   -inf only): such a map has no peak, count 0, agg = the quiet NaN 0x7fc00000 (the reference's 0 / 0); with a NaN the median is
 *   that NaN too.  (The up-sampling gives inf x 0 = NaN for an infinite tap, as ATen's does: a class response map of -inf
 *   reports CIM_PRM_STATUS_NAN.)
 *   One launch.
 * cim_prmt_stim_backward: grad_agg [B, C] f32, count, bitmap (of the forward with the same B, C, h, w, factor) ->
 *   dcrm [B, C, h, w] f32 = sum over the peaks q in row-major order of wy(q) wx(q) (grad_agg / count): the forward's own fp32
 *   tap weights on the forward's own tap pixels, gathered per low-resolution pixel; all 0 for a map without a
 *   peak.  dbias [C] f32 or NULL: the sum of dcrm over the map and the batch, in a second launch.
 * cim_prmt_msm_loss: agg [B, C] f32, target [B, C] f32 in [0, 1] -> loss [1] f32 = torch's multilabel_soft_margin_loss (the mean
 *   over images and classes of -(t logsigmoid(x) + (1 - t) logsigmoid(-x)), softplus form, finite for every finite x) and
 *   dagg [B, C] f32 = (sigmoid(x) - t) / (B C), both written by ONE single-workgroup launch. */
#define CIM_PRM_STIM_MAX_HW 16384
int cim_prmt_stim_forward(const float* crm, const float* bias, int B, int C, int h, int w, int factor, float* agg, int32_t* count,
                          float* median, int32_t* status, uint32_t* bitmap, void* stream);
int cim_prmt_stim_backward(const float* grad_agg, const int32_t* count, const uint32_t* bitmap, int B, int C, int h, int w,
                           int factor, float* dcrm, float* dbias, void* stream);
int cim_prmt_msm_loss(const float* agg, const float* target, int B, int C, float* loss, float* dagg, void* stream);

/* ------------------------------------------------------------------ PRM peak back-propagation: the peak response maps (ABI-16 addition)
 * Replaces what PeakResponseMapping(...).inference() does behind its forward pass (lib/prm/prm_model_gt.py:249-310): every valid
 * peak sent back through convolutions patched by lib/prm/prm_modules.py:104-140 (pr_conv2d: offset o = min x, xs = x - o,
 * n = conv(xs, max(W, 0)), ghat = n < 1e-10 ? 0 : g / (|n| + 1e-10), dx = xs * conv_transpose(ghat, max(W, 0))), P sequential
 * batch-1 passes there; here ONE pass whose batch dimension is the P peaks over tensors of the forward pass that all peaks share.
 * The products are cim_conv1x1_bn_act_bwd / cim_conv3x3_nchw_bn_act_bwd with w = max(W, 0), dy_is_dconv = 1, dw = NULL, B = P;
 * these entries are the stages between them and the stem's data gradient (csrc/prm_backprop.hip).  Stateless, re-entrant on the
 * caller's stream, no atomics, every sum in a fixed order.  Additive: cim_abi_version() stays 16, no new struct.  The entries are
 * named cim_prmb_*: "PRM back-propagation".  Exactness contract and the bytes each launch moves: DESIGN.md 4.25.
 * Every entry refuses (-1, cim_last_error() names the condition) a NULL pointer that is not marked optional and a count < 1.
 *
 * cim_prmb_min: out[0] = the minimum of x[0..n) (NaN is skipped), no host read.  part: cim_prmb_min_parts(n) floats of scratch
 *   (at most CIM_PRMB_MIN_MAX_PARTS).  Two launches.
 * cim_prmb_shift: xs[i] = x[i] - o[0], o a device scalar.  n < 2^31.
 * cim_prmb_gate: g [P, C, HW], and of ONE image: mul [C, HW] (or NULL: the xs of the convolution that produced g as its raw data
 *   gradient; g is taken as mul * g), y [C, HW] (or NULL: no ReLU), a [C] (or NULL: no BatchNorm; a = gamma rsqrt(var + eps), its
 *   sign kept), n [C, HW] ->
 *     t = y > 0 ? g : 0;   dres [P, C, HW] (or NULL) = t;   dconv [P, C, HW] = n < 1e-10 ? 0 : (t * a) / (|n| + 1e-10).
 *   mul, y, a and n are read once per launch, not once per peak.  C HW < 2^31.
 * cim_prmb_scale: dx [P, n] = xs [n] * dxraw [P, n] (+ add [P, n] when given: the gradient that reaches x through another branch).
 * cim_prmb_seed: peaks [P, 3] int32 in DEVICE memory = (class, y, x) on the up-sampled grid (factor h x factor w) ->
 *   dconv [P, C, h, w] of the classifier: the one-hot seed through the adjoint of cim_prm_upsample's own taps (its fp32 weights;
 *   the four products lx ly are added to their tap pixels in the order 00, 01, 10, 11, coinciding taps add up), then the gate
 *   with n [C, h, w] and neither y nor a.  A peak outside the grid or the classes seeds nothing.  P C h w < 2^31.
 * cim_prmb_stem: the data gradient of the 7 x 7 / stride 2 / padding 3 stem convolution with wpos = max(W, 0) [cout][3][7][7],
 *   fused with the multiply by xs [3][H][W], the sum over the 3 input channels and the clamp at 0:
 *     out [P][H][W] = max(0, sum_ci xs[ci][y][x] sum_{co,ky,kx} ghat[p][co][(y + 3 - ky) / 2][(x + 3 - kx) / 2] wpos[co][ci][ky][kx])
 *   over the taps with y + 3 - ky and x + 3 - kx even and inside ghat [P][cout][Ho][Wo], Ho = (H - 1) / 2 + 1.  normalise != 0: a
 *   second launch divides every map by its sum (per-workgroup partial sums in double, added in a fixed order; a zero sum gives
 *   NaN = 0 / 0 as the reference's prm / prm.sum()).  workspace: cim_prmb_stem_workspace(P, H, W) bytes, 8-byte aligned.
 *   cout <= 256, P <= 65535, W <= 4096, H W < 2^22, any H and W. */
#define CIM_PRMB_MIN_MAX_PARTS 1024
long long cim_prmb_min_parts(long long n);
int cim_prmb_min(const float* x, long long n, float* out, float* part, void* stream);
int cim_prmb_shift(const float* x, const float* o, float* xs, long long n, void* stream);
int cim_prmb_gate(const float* g, const float* mul, const float* y, const float* a, const float* n, float* dconv, float* dres,
                  int P, int C, long long HW, void* stream);
int cim_prmb_scale(const float* xs, const float* dxraw, const float* add, float* dx, int P, long long n, void* stream);
int cim_prmb_seed(const int32_t* peaks_dev, const float* n, float* dconv, int P, int C, int h, int w, int factor, void* stream);
long long cim_prmb_stem_workspace(int P, int H, int W);
int cim_prmb_stem(const float* ghat, const float* wpos, const float* xs, float* out, void* workspace, int P, int cout, int H, int W,
                  int normalise, void* stream);

/* ------------------------------------------------------------------ Pillow's antialiased resize: raw RGB images to PRM inputs (ABI-16 addition)
 * Replaces the host call Image.resize((448, 448), Image.BILINEAR) in front of the PRM (tools/pre/AGPL_label_assign.py through
 * prm_configs.open_transform: transforms.Resize([448, 448]), ToTensor, Normalize) for a BATCH of images of differing sizes.
 * Bit-identical to Pillow's src/libImaging/Resample.c on 8-bit RGB (tests/golden/pil_resample_np.py restates it): per axis a table
 * of 22-bit fixed-point coefficients computed in IEEE double, the horizontal pass into a uint8 intermediate, then the vertical
 * pass.  Additive: cim_abi_version() stays 16.  Exactness contract, the refusal and its reason: DESIGN.md 4.20.
 *
 * src: the images' bytes [h][w][3] (RGB, interleaved) anywhere in one device buffer.  desc: int64 [B][3] = (byte offset into
 * src, h, w) per image; the caller passes it twice, desc_host (HOST memory, read and checked before the call returns) and
 * desc_dev (the same words in device memory, read by the kernels).
 * Refused before any launch (-1, cim_last_error() names the condition): B < 1 (or > 65535), a source side outside
 * 1..CIM_RESAMPLE_MAX_SRC, an output side outside 1..CIM_RESAMPLE_MAX_DST, h > CIM_RESAMPLE_MAX_ASPECT w (Pillow runs the
 * vertical pass first there, which changes the bytes), both destinations NULL, an offset before the end of the previous image.
 * ws: cim_resample_ws_bytes(B, desc_host, out_w, out_h) bytes (-1 for a refused batch), 8-byte aligned, no initial content:
 *   inter_off int64 [B] | bounds_x int32 [B][out_w][2] | bounds_y int32 [B][out_h][2] | coef_x int32 [B][out_w][KX] |
 *   coef_y int32 [B][out_h][KY] | the uint8 intermediates [h][out_w][3], image after image;
 *   bounds = (first source index, number of taps), KX / KY = the longest table row of the batch over the widths / heights,
 *   a row of n_in -> n_out samples having 2 ceil(max(n_in / n_out, 1)) + 1 entries (those behind its taps are 0).
 *
 * cim_resample_tables: the table launch alone (one lane per image, axis and output index) into ws.
 * cim_resample_rgb: tables, horizontal pass, vertical pass - three launches for any B, no host synchronisation - writing
 *   dst_u8 [B][out_h][out_w][3] uint8 (Pillow's array) and / or dst_f32 [B][3][out_h][out_w] f32 =
 *   ((float)byte / 255 - mean[c]) / std[c], the arithmetic of cim_image_prep; either may be NULL, not both.
 *   mean_std6_host: six HOST floats (mean RGB, std RGB), needed with dst_f32. */
#define CIM_RESAMPLE_MAX_SRC 16384
#define CIM_RESAMPLE_MAX_DST 4096
#define CIM_RESAMPLE_MAX_ASPECT 100
#define CIM_RESAMPLE_PRECISION_BITS 22
long long cim_resample_ws_bytes(int B, const int64_t* desc_host, int out_w, int out_h);
int cim_resample_tables(const int64_t* desc_host, const int64_t* desc_dev, int B, int out_w, int out_h, void* ws, void* stream);
int cim_resample_rgb(const uint8_t* src, const int64_t* desc_host, const int64_t* desc_dev, int B, int out_w, int out_h,
                     uint8_t* dst_u8, float* dst_f32, const float* mean_std6_host, void* ws, void* stream);

/* ------------------------------------------------------------------ network-input image (f-3: the data side of the step)
 * Replaces prep_im_for_blob(flag="ToTensor"), lib/utils/blob.py:93-147, called from lib/roi_data/minibatch.py:109-150
 * (training) and lib/core/test.py:464-473 via get_image_blob (inference):
 *   src_bgr [h,w,3] uint8 as cv2.imread returns it (device memory) [-> horizontal flip, minibatch.py:121-122]
 *   -> float32 -> cv2.resize(fx = fy = im_scale, INTER_LINEAR) -> np.uint8 -> BGR2RGB -> /255 -> (x - mean) / std
 * dst: float32 planes [3][H][W] of an NCHW blob: element (c,y,x) at dst[c*plane_stride + y*row_stride + x]
 * (H = round(h*im_scale), W = round(w*im_scale); strides let the caller write into a padded batch blob,
 * lib/utils/blob.py:59-83).  inv_scale = 1 / im_scale (double, as cv::resize uses it).
 * mean_std6_host: HOST pointer to {mean_r, mean_g, mean_b, std_r, std_g, std_b}.
 * The resize arithmetic restates OpenCV 4.x's INTER_LINEAR float path; cv2 is not in the reference tree: unpinned. */
int cim_image_prep(const uint8_t* src_bgr, int h, int w, float* dst, int H, int W, long long plane_stride, int row_stride,
                   double inv_scale, int hflip, const float* mean_std6_host, void* stream);

/* ------------------------------------------------------------------ max-pooling / nearest up-sampling of the bodies (a-11)
 * Replaces nn.MaxPool2d(3, 2, 1) of the ResNet stem (lib/modeling/resnet50.py:29, torchvision resnet50.maxpool), nn.MaxPool2d(2, 2)
 * of VGG16 (lib/modeling/vgg16.py:43,50,60) and nn.Upsample(scale_factor = 2^k, mode = 'nearest') of HRNet's fuse layers
 * (lib/modeling/HRNet.py:201).  x: NC planes [H][W] fp32 (NCHW contiguous).  ATen semantics: floor output size
 * (cim_maxpool2d_out_size), no dilation, the window is scanned rows first, the first maximum wins, NaN propagates.
 *   cim_maxpool2d_fwd: y [NC][Ho][Wo]; idx (may be NULL: inference / frozen stem) receives the arg-max as h * W + w
 *   cim_maxpool2d_bwd: dx [NC][H][W] = for every input pixel the sum of dy over the windows whose arg-max it is (a gather in
 *                      window order: deterministic, no atomics)
 *   cim_upsample_nearest_fwd: y [NC][H*scale][W*scale] = x[.., oh / scale, ow / scale]; accumulate != 0: y += ... (the fuse sum)
 *   cim_upsample_nearest_bwd: dx [NC][H][W] = sum of the scale x scale block of dy, rows first */
int cim_maxpool2d_out_size(int in, int k, int stride, int pad);
int cim_maxpool2d_fwd(const float* x, float* y, int* idx, int NC, int H, int W, int k, int stride, int pad, void* stream);
int cim_maxpool2d_bwd(const float* dy, const int* idx, float* dx, int NC, int H, int W, int k, int stride, int pad, void* stream);
int cim_upsample_nearest_fwd(const float* x, float* y, int NC, int H, int W, int scale, int accumulate, void* stream);
int cim_upsample_nearest_bwd(const float* dy, float* dx, int NC, int H, int W, int scale, void* stream);

/* ------------------------------------------------------------------ backbone 1x1 convolutions (a-11)
 * The 1 x 1 convolutions of the ResNet bottlenecks (torchvision Bottleneck conv1 / conv3 / downsample.0 as wrapped by
 * lib/modeling/resnet50.py:17-91) and their backward products as small-tile fp32-MFMA GEMMs, C[M,N] = A . B:
 *   A: a_mcontig == 0: element (m,k) at A[m*lda + k];  1: at A[k*lda + m]
 *   B: b_kcontig == 0: element (k,n) at B[k*ldb + n];  1: at B[n*ldb + k]
 *   forward (NCHW, one image): A = weight [Cout][Cin], B = x [Cin][HW];  dX: A = weight (a_mcontig), B = dy;
 *   dW: A = dy [Cout][HW], B = x [Cin][HW] (b_kcontig).
 * Epilogue (splits == 1): x_raw (optional) receives the plain product (the convolution output the BatchNorm backward
 * needs); C = relu?(acc * a[m] + b[m] (+ residual)), a = gamma*rsqrt(var+eps), b = beta - mean*a per ROW m (= output
 * channel) when gamma/beta/mean/var are given - the frozen-statistics BatchNorm (+ identity) (+ ReLU) that follows the
 * convolution, lib/modeling/resnet50.py:53-77 - else C = relu?(acc (+ residual)).
 * splits > 1 (cim_gemm_small_splits): split-K through `workspace` [splits][M][N] + a fixed-order reduce pass that applies
 * the same epilogue. */
int cim_gemm_small_splits(int M, int N, int K);
int cim_gemm_small_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                       int a_mcontig, int b_kcontig, float* x_raw, const float* gamma, const float* beta,
                       const float* mean, const float* var, float eps, const float* residual, int relu, int splits,
                       float* workspace, void* stream);

/* Backward of conv1x1 -> frozen BatchNorm (+ residual) (+ ReLU) for B images in one call: BatchNorm / ReLU backward
 * (cim_bn_act_bwd), dx [B,cin,hw] = W^T . dconv, dw [cout,cin] = sum_b dconv_b . x_b^T.  dy, y (post-activation output; may
 * be NULL without relu), x_raw (convolution output) are [B,cout,hw]; x is the convolution input [B,cin,hw]; w [cout,cin].
 * dres / dgamma+dbeta / dx / dw may be NULL when not needed.  workspace: cim_conv1x1_bwd_workspace(B,cin,cout,hw) bytes.
 * side_stream (may be NULL): a second HIP stream the weight-gradient GEMM is enqueued on, next to the data-gradient GEMM on
 * `stream`, forked after the BatchNorm backward through fork_event (a hipEvent_t of the CALLER, created with
 * hipEventDisableTiming, passed as void*; needed whenever side_stream is given - the library creates no events).  join != 0:
 * `stream` waits for it through join_event (the caller's as well) before the call returns (stream order is all the
 * caller needs); join == 0: the CALLER makes `stream` wait for side_stream before dw (and the buffers x, workspace) are used or
 * reused - the weight gradients of a whole backward pass then run beside the data-gradient chain.  Both events are recorded and
 * waited on inside the call: the caller may pass the same pair to its next call.
 * Chaining two layers' backward without a BatchNorm-backward launch in between (round 3):
 *   in_gamma, in_var, in_eps (in_gamma may be NULL): frozen BatchNorm of the layer that PRODUCED x as relu(bn(conv)) with no
 *     residual - dx is then written as  x > 0 ? dx * in_gamma rsqrt(in_var + in_eps) : 0,  i.e. already the gradient of that
 *     layer's convolution output (its BatchNorm + ReLU backward in this product's epilogue);
 *   dy_is_dconv != 0: dy IS such a gradient of this layer's convolution output (handed over by the layer after it): the
 *     BatchNorm backward launch is skipped (dres must be NULL).
 * With TRAINABLE gamma / beta in the producing layer (the reference's configuration: lib/modeling/resnet50.py:59-60 leaves the
 * affine parameters of the frozen-statistics BatchNorm layers trainable) (round 4):
 *   in_xr, in_mean, in_part (in_part may be NULL): that layer's convolution output [B,cin,hw], its running mean, and
 *     [B][2][ceil(hw/32)][cin] floats that receive, per 32-pixel group g of every channel c, sum dz and sum dz (in_xr - in_mean)
 *     over the group (dz = x > 0 ? dx : 0) - the per-channel sums of that layer's BatchNorm backward, written by the same epilogue;
 *   a layer called with dy_is_dconv gets its own dgamma / dbeta from the array its consumer filled: cim_bn_part_finish below
 *     (dgamma, dbeta must be NULL in that call). */
long long cim_conv1x1_bwd_workspace(int B, int cin, int cout, int hw);
int cim_conv1x1_bn_act_bwd(const float* dy, const float* y, const float* x_raw, const float* x, const float* w,
                           const float* gamma, const float* mean, const float* var, float eps, int relu,
                           float* dres, float* dgamma, float* dbeta, float* dx, float* dw, int B, int cin, int cout, int hw,
                           float* workspace, void* stream, void* side_stream, void* fork_event, void* join_event, int join,
                           int dy_is_dconv, const float* in_gamma, const float* in_var, float in_eps,
                           const float* in_xr, const float* in_mean, float* in_part, const float* dx_add, int dx_add_w);
/* dx_add (may be NULL; round 4): [B,cin,hw] added to dx in the data gradient's epilogue - the gradient that reaches x through a
 * SECOND branch (the identity path of a bottleneck: lib/modeling/resnet50.py:17-44 torchvision Bottleneck `out += identity`, or
 * the block's downsample convolution), so that autograd needs no separate add launch per block.
 * dx_add_w = 0: dx_add has dx's shape.  dx_add_w = W > 0 (hw = H W): dx_add is [B,cin,ceil(H/2),ceil(W/2)], the data gradient of
 * a STRIDE-2 1 x 1 convolution of the same x - added at the pixels (2i, 2j) it belongs to (replaces autograd's zero-filled
 * scatter of the strided slice: two fills, two copies and an add per downsample block).
 * The affine gradients of chained layers from those partial sums, for n layers in ceil(n / 24) launches (`descs` is a HOST array):
 * dbeta[c] = sum over images and groups of part[b][0][g][c], dgamma[c] = rsqrt(var[c] + eps) sum part[b][1][g][c], in index
 * order (deterministic).  dgamma or dbeta may be NULL.  One call at the end of a backward pass serves the whole body. */
typedef struct { const float* part; const float* var; float eps; float* dgamma; float* dbeta; int images; int parts; int channels; } cim_bn_part_desc;
int cim_bn_part_finish(const cim_bn_part_desc* descs, int n, void* stream);

/* 3 x 3 convolution (padding 1, stride 1 or 2, no bias, groups 1) -> frozen BatchNorm (+ residual) (+ ReLU) of the
 * bottlenecks (torchvision Bottleneck.conv2 / bn2, lib/modeling/resnet50.py:17-44,53-77), NCHW fp32, ONE image per call, as an
 * implicit GEMM on the small-tile fp32-MFMA kernel above (the im2col matrix is never built): x [cin][H][W], w [cout][cin][3][3]
 * (the nn.Conv2d weight as it is), y / x_raw / residual [cout][Ho][Wo], Ho = (H-1)/stride + 1.  Epilogue and split-K as
 * cim_gemm_small_f32 (workspace [splits][cout][Ho Wo] floats when cim_conv3x3_nchw_splits(...) > 1).  cin % 4 == 0.
 * Replaces ATen -> MIOpen (miopenSp3AsmConv / Im2d2Col + rocBLAS) for those layers. */
int cim_conv3x3_nchw_splits(int cin, int cout, int H, int W, int stride);
int cim_conv3x3_nchw_f32(const float* x, const float* w, float* y, int cin, int cout, int H, int W, int stride, int dilation,
                         float* x_raw, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                         const float* residual, int relu, int splits, float* workspace, void* stream);
/* dilation >= 1 with padding = dilation ("same"; dilation > 1 needs stride 1): the dilated conv5 of VGG16
 * (lib/modeling/vgg16.py:70-78).  A convolution with a bias and no BatchNorm is the same call with gamma = 1, beta = bias,
 * mean = 0, var = 1, eps = 0 (a = 1 exactly); a bias in front of a BatchNorm is folded into mean (mean - bias).  The forward
 * takes any cin (the frozen RGB stems); the backward needs cin % 4 == 0. */
/* The stem of the ResNet body: 7 x 7 convolution (padding 3, stride 1 or 2, no bias, any cin) -> frozen BatchNorm (+ ReLU),
 * forward only (torchvision ResNet conv1 / bn1 / relu, lib/modeling/resnet50.py:20,53-77, frozen by FREEZE_AT): the same
 * implicit GEMM with 49 taps.  x [cin][H][W], w [cout][cin][7][7], y [cout][Ho][Wo].  Replaces ATen -> MIOpen + 2 launches. */
int cim_conv7x7_nchw_f32(const float* x, const float* w, float* y, int cin, int cout, int H, int W, int stride,
                         const float* gamma, const float* beta, const float* mean, const float* var, float eps, int relu,
                         void* stream);
/* Backward of cim_conv3x3_nchw_f32 for B images in one call: BatchNorm / ReLU backward (cim_bn_act_bwd), dx [B,cin,H,W] (transposed
 * convolution as an implicit GEMM over (cout, tap)), dw [cout,cin,3,3] = sum over images and output pixels (split-K).
 * dy, y (may be NULL without relu), x_raw are [B,cout,Ho,Wo]; dres / dgamma+dbeta / dx / dw may be NULL when not needed.
 * workspace: cim_conv3x3_nchw_bwd_workspace(...) bytes.  cin % 4 == 0, cout % 4 == 0.  side_stream, fork_event, join_event, join,
 * dy_is_dconv and in_gamma / in_var / in_eps as in cim_conv1x1_bn_act_bwd. */
long long cim_conv3x3_nchw_bwd_workspace(int B, int cin, int cout, int H, int W, int stride);
/* cim_conv3x3_dx_parts (ABI 14): the number of 32-pixel groups `in_part` ([B][2][parts][cin]) must provide for this geometry - stride 1:
 * ceil(H W / 32); stride 2 (dilation 1): the data gradient runs by parity classes of the input pixels (a class only contracts over
 * the taps that reach it: 9 of the 36 (tap, class) pairs) and numbers its groups class by class, tile padded. */
int cim_conv3x3_dx_parts(int H, int W, int stride);
int cim_conv3x3_nchw_bn_act_bwd(const float* dy, const float* y, const float* x_raw, const float* x, const float* w,
                                const float* gamma, const float* mean, const float* var, float eps, int relu, float* dres,
                                float* dgamma, float* dbeta, float* dx, float* dw, int B, int cin, int cout, int H, int W,
                                int stride, int dilation, float* workspace, void* stream, void* side_stream, void* fork_event,
                                void* join_event, int join, int dy_is_dconv, const float* in_gamma, const float* in_var, float in_eps,
                                const float* in_xr, const float* in_mean, float* in_part, const float* wt_ready);
/* wt_ready (may be NULL): the weight transposed to [cout][3][3][cin] - the data gradient's A operand - when the caller made it
 * ahead of the pass; else the call makes it itself (one small launch per layer in front of the data gradient).
 * cim_conv3x3_wt_multi: those transposes for n layers in ceil(n / 16) launches (`descs` is a HOST array; weights only change at
 * the optimizer step, so a body's transposes are made once per step beside the forward pass). */
typedef struct { const float* w; float* wt; int cin; int cout; } cim_wt_desc;
int cim_conv3x3_wt_multi(const cim_wt_desc* descs, int n, void* stream);

/* Weight gradient of the 7 x 7 stem convolution (padding 3, stride 1 or 2, no bias; torchvision ResNet conv1 with FREEZE_AT = 0,
 * lib/modeling/resnet50.py, and lib/prm/prm_model.py fc_resnet50, whose stem trains), B images in one call (csrc/conv7x7_dw.hip):
 *   dw[co][ci][ky][kx] = sum over b, oy, ox of dconv[b][co][oy][ox] * x[b][ci][oy stride + ky - 3][ox stride + kx - 3]
 * dconv [B][cout][Ho][Wo] is the gradient of the convolution's output (what cim_bn_act_bwd leaves as dx), Ho = (H-1)/stride + 1;
 * x [B][cin][H][W]; dw [cout][cin][7][7] is WRITTEN, not accumulated.  True fp32 products on the matrix pipe; partial sums of
 * fixed sets of output pixels go to workspace as [splits][cout][cin 49] and a second launch adds them in a fixed order: no
 * atomics, the same bits on every call.  workspace: cim_conv7x7_dw_workspace(...) bytes, the caller's; cim_conv7x7_dw_splits is a
 * function of the shape alone.  1 <= cin <= 4, 1 <= cout <= 256, W <= 4096, H W < 2^20; anything else returns -1 before a launch.
 * Replaces ATen -> MIOpen's convolution weight gradient for that layer. */
long long cim_conv7x7_dw_workspace(int B, int cin, int cout, int H, int W, int stride);
int cim_conv7x7_dw_splits(int B, int cin, int cout, int H, int W, int stride);
int cim_conv7x7_dw_f32(const float* dconv, const float* x, float* dw, int B, int cin, int cout, int H, int W, int stride,
                       float* workspace, void* stream);

/* ------------------------------------------------------------------ backbone BatchNorm chains (a-11)
 * Frozen-statistics BatchNorm (+ residual) (+ ReLU) of the ResNet / HRNet bodies, lib/modeling/resnet50.py:17-44,53-77
 * (every BN in eval(): running statistics, trainable affine), one launch each way instead of 2-3 / 3-4 ATen passes.
 * NCHW fp32; x, res, y, dy, dx, dres are [N,C,HW]; gamma, beta, mean, var, dgamma, dbeta are [C].
 *   fwd: y = relu?(x*a + b (+ res)),  a = gamma*rsqrt(var+eps),  b = beta - mean*a        (res may be NULL)
 *   bwd: dz = dy*(y>0 if relu); dx = dz*a; dres = dz; dgamma = sum dz*(x-mean)*rstd; dbeta = sum dz
 *        (dx, dres, and the dgamma/dbeta pair may be NULL when not needed; y may be NULL without relu).
 *        When cim_bn_act_bwd_chunks(N,C,HW) > 1 the per-channel sums are accumulated with atomicAdd: the caller
 *        zeroes dgamma / dbeta first. */
int cim_bn_act_fwd(const float* x, const float* res, const float* gamma, const float* beta, const float* mean,
                   const float* var, float eps, float* y, int N, int C, int HW, int relu, void* stream);
int cim_bn_act_bwd_chunks(int N, int C, int HW);
int cim_bn_act_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean,
                   const float* var, float eps, float* dx, float* dres, float* dgamma, float* dbeta,
                   int N, int C, int HW, int relu, void* stream);

/* Batch-statistics BatchNorm (+ residual) (+ ReLU): nn.BatchNorm2d in train() mode (csrc/bn_train.hip; ABI-16 addition:
 * cim_abi_version() stays 16).  What lib/prm/prm_model.py's PeakResponseMapping.train() runs in every BatchNorm of its network.
 * Layout as above, m = N HW values per channel.  A channel's values are cut into cim_bn_train_chunks(N,C,HW) chunks, a function of
 * the shape alone; per-chunk partials go to workspace (cim_bn_train_workspace(N,C,HW) bytes, the caller's, 8-byte aligned, the same
 * size for both calls) and a finishing launch adds them in a fixed order, in double: no atomics, the same bits on every call.
 *   fwd: mean, var (biased; centred sums joined with Chan's formula) and, when rstd != NULL, rstd = rsqrtf(var + eps) are WRITTEN;
 *        y = cim_bn_act_fwd(x, res, gamma, beta, mean, var, eps), bit for bit (it is that call).  With running_mean / running_var
 *        (both or neither):  running_mean = (1 - f) running_mean + f mean,  running_var = (1 - f) running_var + f var m / (m - 1),
 *        f = momentum, or, momentum < 0 (torch's momentum None), 1 / *num_batches_tracked AFTER its increment.
 *        *num_batches_tracked (int64 device word, may be NULL unless momentum < 0 with running buffers) += 1, an ordinary store.
 *   bwd (sums and dx computed in double): dz = dy*(y>0 if relu);  S1 = sum dz, S2 = sum dz (x - mean);  dbeta = S1, dgamma = rstd S2 (both or neither);
 *        dx = gamma rstd (dz - S1 / m - (x - mean) rstd^2 S2 / m), dres = dz (each may be NULL); y may be NULL without relu.
 * 16-byte accesses when every tensor's base is 16-byte aligned, else scalar ones.  C < 1, N HW < 2 (torch: "Expected more than 1
 * value per channel when training"), N C HW > INT_MAX or a NULL required pointer return -1 before any launch; the two size
 * entries return -1 for such a shape. */
long long cim_bn_train_workspace(int N, int C, int HW);
long long cim_bn_train_chunks(int N, int C, int HW);
int cim_bn_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, long long* num_batches_tracked, float* y, float* mean, float* var,
                     float* rstd, int N, int C, int HW, int relu, float* workspace, void* stream);
int cim_bn_train_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean, const float* rstd,
                     float* dx, float* dres, float* dgamma, float* dbeta, int N, int C, int HW, int relu, float* workspace,
                     void* stream);

/* ------------------------------------------------------------------ MaskFuse contractions (a-2)
 * The dense contractions behind MaskFuse, lib/modeling/resnet50.py:104-110,135-136 (Conv2d(2C,C,3,pad=1) in the mixed 4 + 3
 * Winograd tiling of the 7 x 7 ROI map, Linear(49C,4096), Linear(4096,4096)) and their autograd backward: fp32 in, fp32 out, on
 * ONE arithmetic engine and ONE convolution algorithm.  (Rounds 1-3 carried four engines and four algorithms behind environment
 * switches; the superseded ones are test infrastructure now: experiments/include/cim_exp.h.)
 */
/* The pair engine ("f16x2p"): every fp32 operand x is scaled by ONE power of two per matrix and split into two fp16 terms,
 * x * s = h + l (22 significant bits); a product is evaluated as h*l + l*h + h*h on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation and rescaled exactly in the epilogue (error class of an fp32 GEMM, tests/test_gpu_gemm_pair.py).  The operands were split by
 * their PRODUCERS.  A "pair image" of a logical fp32 matrix [rows][cols] is [rows][ld / 8][h: 8 x f16 | l: 8 x f16]
 * (ld logical elements per row, a multiple of 8; 4 bytes per element) with x * s = h + l for ONE power-of-two scale s per
 * matrix (per batch entry).  The same image serves the product that contracts over its columns (K-contiguous use) and the
 * one that contracts over its rows (through the hardware transpose read of LDS), so it is written once.  The GEMM moves
 * 16-byte chunks HBM -> LDS by LDS-DMA; its loop holds MFMAs and LDS reads only.
 *   cim_gemm_pair[_batched]: C[M,N] = A . B * 1 / (a_scale * b_scale) (+ bias)(ReLU), fp32 C.  a_mcontig = 0: A element (m,k) at A[m*lda + k], 1: at A[k*lda + m]; b_kcontig = 0: B element (k,n) at B[k*ldb + n], 1: at B[n*ldb + k];
 *     K % 32 == 0 (zero-filled rows / columns pad the images), lda / ldb % 8 == 0, an M-contiguous A needs M % 8 == 0, an
 *     N-contiguous B needs N % 8 == 0.  a_scale / b_scale: [batch] device floats, the scales the images were written with.
 *     c_amax (optional): receives max |C| as an IEEE bit pattern through atomicMax (caller zeroes) - the scale source
 *     of the next split.  With splits > 1 and K > 32 the split-K reduce moves 16 bytes per lane: C, workspace (splits * M * N
 *     floats) and a non-NULL bias must then be 16-byte aligned (ldc % 4 == 0 always).
 *   cim_pair_scales: scale[i] = 2^(14 - exponent(amax[min(i, n_amax - 1)] * factor[i]))  (factor may be NULL); reduce_all != 0:
 *                    every scale from the MAXIMUM of the n_amax words (row / column maxima of a weight -> its one scale)
 *   cim_pair_split : fp32 X [batch][rows][ld] -> pair image [batch][rows_pad][ldp], rows >= `rows` zero-filled; relu_y
 *                    (optional, laid out as X): elements with relu_y <= 0 are written as 0 (a fused ReLU backward mask)
 *   cim_pair_amax  : max |x| bit pattern of n floats (atomicMax into a caller-zeroed word; X 16-byte aligned, any n)
 *   cim_pair_masked_stats: the ReLU backward of a fully connected layer in front of its split, dz = y > 0 ? dy : 0 on [rows][cols]
 *                    (never stored: cim_pair_split applies the same mask): max |dz| as cim_pair_amax and, when `part`
 *                    ([ceil(rows / 64)][cols], may be NULL) is given, the bias gradient's partial sums over chunks of 64 rows, each
 *                    added up in row order - the caller sums the chunks (lib/modeling/resnet50.py:107-110 seg_fc's ReLUs) */
/* max_workgroups (0 = one launch over all tiles): caps the launches of THIS product - it then goes out as consecutive launches
 * of at most that many workgroups.  A workgroup of this engine owns its CU (128 KB of LDS), so a capped product never holds
 * more CUs than that and leaves the rest of the chip to concurrent streams - used for the MaskFuse weight-gradient products
 * that run beside the backbone's backward (cim_amd/ops/maskfuse_pair.py).  Same tiles, same arithmetic, same bits. */
/* products: 3 = the fp32-class evaluation h*l + l*h + h*h (the training step's arithmetic); 1 = the h*h product alone - operands
 * with 11 significant bits, fp32 accumulation: the arithmetic class of TF32, which the reference's own convolutions / matmuls
 * run in on its hardware (torch 1.10 defaults; tools/train.py:153-154 touches cudnn.deterministic / benchmark only).  Reported
 * beside the headline as bench.py's extra.tf32_class, never used by default. */
/* form: 0 = 256 x 256 tiles, eight waves, 128 KB of LDS - a workgroup owns its CU (every product of the forward / data-gradient
 * chains); 1 = 128 x 256 tiles, four waves (one per SIMD, <= 256 registers each), 96 KB of LDS: half of the CU's registers and 64 KB of
 * its LDS stay free, so workgroups of kernels on OTHER streams run on the same CU beside it - the form of the MaskFuse weight
 * gradients that run beside the backbone's backward (a_mcontig = 1, b_kcontig = 0 only).  Same products in the same order per
 * output element: same bits as form 0. */
int cim_gemm_pair_splits(int M, int N, int K);
int cim_gemm_pair(const void* A, const void* B, float* C, const float* bias, int M, int N, int K,
                  int lda, int ldb, int ldc, int a_mcontig, int b_kcontig, int relu, int splits, float* workspace,
                  const float* a_scale, const float* b_scale, uint32_t* c_amax, int max_workgroups, int products, int form,
                  void* stream);
int cim_gemm_pair_batched(const void* A, const void* B, float* C, int M, int N, int K,
                          int lda, int ldb, int ldc, int a_mcontig, int b_kcontig,
                          int batch, long long a_bs, long long b_bs, long long c_bs,
                          const float* a_scale, const float* b_scale, int max_workgroups, int products, int form, void* stream);
int cim_pair_scales(const uint32_t* amax, int n_amax, const float* factor, float* scale, int n, int reduce_all, void* stream);
int cim_pair_split(const float* X, void* P, int rows, int rows_pad, int cols, int ld, int ldp, int batch,
                   long long x_bs, long long p_bs, const float* scale, const float* relu_y, void* stream);
int cim_pair_amax(const float* X, long long n, uint32_t* amax, void* stream);
int cim_pair_masked_stats(const float* dy, const float* y, int rows, int cols, float* part, uint32_t* amax, void* stream);

/* Producers of pair images for the MaskFuse convolution in the mixed 4 + 3 Winograd tiling (121 positions, P = 7) and for seg_fc.0's input:
 *   cim_wino7_pair_scales: scale[121] from max |d| of the untransformed tensor (the maximum of the n_amax bit patterns `amax`, times
 *        max(1, amax_mul[0]) when amax_mul is given: the {0, 1} masks of MaskFuse's concat): per position the bound
 *        (abs row sum)_i (abs row sum)_j max|d| of the transform.  kind 0: input (B^T), 1: filter (G), 2: dy for the weight
 *        gradient (GD), 3: dy for the adjoint data gradient (A)
 *   cim_wino7_input_pair : x [R,7,7,C] fp32 -> V [121][Rs][C] pair image (Rs >= R rows per position, rows >= R zeroed)
 *   cim_wino7_filter_pair: W [Cout,Cin,3,3] -> U' [121][Cout][Cin] pair image (ci contiguous)
 *   cim_wino7_dy_pair    : dy [R,7,7,C] -> D (adjoint = 0: GD dy GD^T) or E (adjoint = 1: A dy A^T) [121][Rs][C]
 *   cim_wino7_flatten_bwd_dy_pair: the backward of the (c, h, w) flatten + mask_branch's ReLU + BOTH transforms above in one launch:
 *        dX [R][C*49] (seg_fc.0's data gradient), relu_y [R,7,7,C] (saved conv output; NULL: no mask) -> E (adjoint = 1 image, may be
 *        NULL) and D (adjoint = 0 image, may be NULL), bit-identical to cim_flatten_chw_bwd_bias + cim_wino7_dy_pair x 2 without the
 *        masked gradient ever being stored; bias_partial [R][C] (may be NULL) as cim_flatten_chw_bwd_bias.  C % 256 == 0
 *   cim_wino7_output_amax: M [121][R][C] -> y [R,7,7,C] = A^T m A per tile (+ bias, ReLU); also reports max |y| (atomicMax, caller zeroes)
 *   cim_flatten_chw_pair : the (c, h, w) flatten of the NCHW `.view(N, -1)` on channels-last data, into a pair image [Rs][C*PP] (lib/modeling/resnet50.py:135) */
int cim_wino7_pair_scales(const uint32_t* amax, int n_amax, const uint32_t* amax_mul, int kind, float* scale, void* stream);
int cim_wino7_input_pair(const float* x, void* V, const float* scale, int R, int Rs, int C, void* stream);
int cim_wino7_filter_pair(const float* W, void* U, const float* scale, int Cout, int Cin, void* stream);
int cim_wino7_dy_pair(const float* dy, void* D, const float* scale, int R, int Rs, int C, int adjoint, void* stream);
int cim_wino7_flatten_bwd_dy_pair(const float* dX, const float* relu_y, void* E, const float* scale_e, void* D, const float* scale_d,
                                  float* bias_partial, int R, int Rs, int C, void* stream);
int cim_wino7_output_amax(const float* M, const float* bias, float* y, int R, int C, int relu, uint32_t* y_amax, void* stream);
int cim_flatten_chw_pair(const float* src, void* dst, const float* scale, int R, int Rs, int PP, int C, void* stream);
/* the flatten's backward: src [R][C][PP] -> dst [R][PP][C], zeroed where relu_y [R][PP][C] <= 0 (the conv's ReLU mask); also writes bias_partial [R][C] = sum over the PP pixels of the masked gradient (the
 * conv's bias gradient is its sum over R); bias_partial may be NULL */
int cim_flatten_chw_bwd_bias(const float* src, const float* relu_y, float* dst, float* bias_partial, int R, int PP, int C,
                             void* stream);


/* fp32 stages of the same tiling that the pair engine's results pass through (tile must be 7):
 *   cim_wino_wgrad_output     : dU [121][Cin][Cout] (fp32, from cim_gemm_pair_batched) -> dW [Cout,Cin,3,3]
 *   cim_wino_dx_adjoint_output: Md [121][R][Cin] -> dx [R,7,7,Cin]   (overlap-add of B Md B^T: the adjoint of the forward) */
int cim_wino_wgrad_output(const float* dU, float* dW, int Cout, int Cin, int tile, void* stream);
int cim_wino_dx_adjoint_output(const float* M, float* dx, int R, int P, int C, int tile, void* stream);
/* cim_wino_dx_adjoint_output (tile = 7) with the backward of MaskFuse's prologue folded in: Md [121][R][2 Cb] is the Winograd-domain
 * gradient of cat = [box, box * mask] (lib/modeling/resnet50.py:131-134); written is  dbox [R,7,7,Cb] = dcat[..., :Cb] + mask *
 * dcat[..., Cb:]  (masks [R,7,7]) - the input of the plain ROIAlign backward (cim_roi_align_bwd_ws), half the bytes of dcat. */
int cim_wino7_dx_maskfold(const float* M, const float* masks, float* dbox, int R, int Cb, void* stream);

/* ------------------------------------------------------------------ losses (a-8, a-9, a-10)
 * Replaces cls_iou_loss + loss_weight_bag_loss (per refinement layer), mil_bag_loss and PCL_loss,
 * lib/modeling/heads.py:10-166, as summed by lib/modeling/model_builder.py:170-204.
 * One launch: R (= REFINE_TIMES <= 3) + 2 workgroups.  All score tensors are [N, C1] f32.
 *   part [R+2][4]  per-job partial losses in the order {bag, pcl, cls, iou}: rows 0..R-1 = the
 *                  refinement layers (iou NOT yet multiplied by 3), row R = mil_bag, row R+1 = PCL
 *   grad [3 + 4R][N][C1]  gradient components for a unit upstream gradient:
 *        0: d bag(mil)/d predict_cls   1: d pcl/d predict_cls   2: d bag(mil)/d predict_det
 *        3+4i: d cls_i/d refine_cls[i]   4+4i: d bag_i/d refine_cls[i]
 *        5+4i: d iou_i/d refine_iou[i]   6+4i: d bag_i/d refine_iou[i]
 * The PCL cluster structure of `mat` (heads.py:14-21: distinct non-zero ids ascending, member rows, the column of each
 * row's entry, the background cluster = the id found in column 0) is derived inside the launch by the PCL workgroup:
 * no host copy of `mat`, no per-image plan.  layer_valid comes straight from cim_mining_step. */
#define CIM_PCL_MAX_CLUSTERS 256
typedef struct cim_loss_args {
    const float* pc;                 /* predict_cls */
    const float* pd;                 /* predict_det */
    const float* rc[3];              /* refine_cls[i] */
    const float* ri[3];              /* refine_iou[i] */
    const float* pseudo_labels[3];   /* [N,C1] one-hot / zero rows (CIM_layer output) */
    const uint16_t* pseudo_iou_f16[3]; /* [N] binary16 {0,1} */
    const float* loss_weights[3];    /* [N] (unscaled) */
    float weight_scale[3];           /* lmda: 3 for layer 0, else 1 (model_builder.py:172) */
    const int32_t* layer_valid;      /* DEVICE [R]: 0 = CIM_layer found no pseudo GT -> layer skipped (cim_mining_step) */
    const float* labels;             /* [C1-1] image labels */
    const float* mat;                /* [N,C1] PRM cluster matrix (heads.py:10-41): <= 1 non-zero (= cluster id) per row */
    int32_t* status;                 /* DEVICE [1] error bits, OR-ed: 4 = a row of mat has several non-zeros (use the
                                        general ATen formulation), 8 = several distinct ids in column 0 (heads.py:20),
                                        16 = more than CIM_PCL_MAX_CLUSTERS clusters */
    int N, C1, R;
    float* part;
    float* grad;
    int ld;                          /* row stride (floats) of pc / pd / rc / ri: C1 (or 0) for dense [N,C1] tensors, 8 C1 when
                                        they are the column blocks of the heads' fused score matrix [N, (2 + 2R) C1] */
} cim_loss_args;

int cim_losses_fwd(const cim_loss_args* args, void* stream);

/* ------------------------------------------------------------------ head activations (a-3)
 * Replaces the softmax / sigmoid epilogue of cls_iou_model.forward, lib/modeling/heads.py:199-217.
 * logits / scores [N, (2+2R)*C1] with column blocks [classifier | detector | refine_cls[R] | refine_iou[R]]:
 * softmax over classes (classifier, refine_cls), softmax over PROPOSALS (detector), sigmoid (refine_iou).
 * colstat / coldot: [2*C1] / [C1] f32 scratch for the detector's column reductions. */
/* The linear part of the eight heads on the small-tile fp32-MFMA GEMM (no library GEMM on the path):
 *   cim_linear_bias_f32: Y[M][N] = X[M][K] . W[N][K]^T + bias[N]   (splits: cim_gemm_small_splits(M, N, K))
 * cim_loss_finish: cim_losses_fwd's partial sums part[rows][4] -> out[6] = (bag, pcl, cls, iou, 3 iou, total) on the device, with
 *   total = ((bag + pcl) + cls) + 3 iou: the IoU loss's weight of lib/modeling/model_builder.py:199 and the sum the driver
 *   differentiates (lib/utils/training_stats.py:72-83 `total_loss += loss` in dictionary order) in the same launch.
 * cim_loss_grad_combine: the gradient of the losses w.r.t. the fused score matrix [N][(2 + 2R) C1] from cim_losses_fwd's `grad`
 *   components and the upstream gradients of cim_loss_finish's six outputs (device scalars; NULL = zero). */
int cim_linear_bias_f32(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, int splits,
                        float* workspace, void* stream);
int cim_loss_finish(const float* part, int rows, float* out, void* stream);
int cim_loss_grad_combine(const float* G, const float* g_bag, const float* g_pcl, const float* g_cls, const float* g_iou,
                          const float* g_iou3, const float* g_total, float* out, int N, int C1, int R, void* stream);
int cim_head_act_fwd(const float* logits, float* scores, float* colstat, int N, int C1, int R, void* stream);
int cim_head_act_bwd(const float* scores, const float* grad_scores, float* grad_logits, float* coldot,
                     int N, int C1, int R, void* stream);

/* ------------------------------------------------------------------ optimizer step
 * Fused multi-tensor SGD with momentum and weight decay: torch.optim.SGD's update (dampening 0, no Nesterov) as
 * constructed at tools/train.py:282-311 and stepped at :438, ONE launch for all tensors:
 *     g' = g + wd*p ;  buf = momentum*buf + g' ;  p = p - lr*buf        (buf zero-initialised by the caller)
 * `tensors` and `chunks` are DEVICE arrays: one record per tensor (refreshed whenever a pointer, lr or wd changes) and one
 * per chunk of a tensor (the host uses 16384-element chunks; offsets are multiples of 4 elements); a workgroup streams
 * one chunk.  16-byte accesses are used when the three pointers of a tensor are 16-byte aligned. */
typedef struct cim_sgd_tensor {
    uint64_t p;        /* float* parameter (device address) */
    uint64_t g;        /* const float* gradient */
    uint64_t buf;      /* float* momentum buffer */
    int64_t n;         /* elements */
    float lr, wd;
    /* matrix mode (cols > 0): the tensor is a [rows][cols] matrix (cols % 4 == 0, 16-byte aligned pointers), its chunks are
     * 64-row x 1024-column tiles (chunk.offset = first row, chunk.n = first column) and the launch also accumulates
     * max |w_new| per row / per column (IEEE bit patterns, atomicMax) into the caller-zeroed arrays row_amax [rows] /
     * col_amax [cols] - the operand scales of the f16x2 contraction engine (cim_amax_rowcol) as a by-product. */
    int32_t rows, cols;
    uint64_t row_amax, col_amax;
} cim_sgd_tensor;
typedef struct cim_sgd_chunk {
    int32_t tensor;    /* index into `tensors` */
    int32_t n;         /* elements of this chunk (clamped to the tensor's end in the kernel) */
    int64_t offset;    /* first element */
} cim_sgd_chunk;
/* max_workgroups (ABI 14): 0 = one workgroup per chunk; > 0: at most that many workgroups, each walking over chunks b, b + grid, ...
 * (an update that runs beside another stream's latency-bound launches holds one or two workgroup slots per CU instead of all). */
int cim_sgd_multi(const cim_sgd_tensor* tensors, const cim_sgd_chunk* chunks, int n_chunks, float momentum, int max_workgroups,
                  void* stream);

/* Fused multi-tensor Adam (ABI-16 addition: cim_abi_version() stays 16): torch.optim.Adam's update with L2 weight decay
 * (no amsgrad, no maximize) as constructed at tools/train.py:310-311, ONE launch for all tensors, in fp32:
 *     g' = fma(wd, p, g)
 *     m  = fma(beta1, m, (1 - beta1) * g')
 *     v  = fma(beta2, v, (1 - beta2) * (g' * g'))
 *     p  = p - (step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 * sqrt and both divisions are the correctly rounded fp32 operations.  beta1, beta2 and eps are doubles: beta and 1 - beta are
 * each rounded to fp32 ONCE, from the double (1 - 0.999f is 1.3e-5 off 0.001: hundreds of ulps of every exp_avg_sq).
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) are per TENSOR (each has its own step count t) and
 * computed by the caller in double precision.  Same two device tables, chunk meaning (16384-element flat chunks, 64 x 1024
 * matrix tiles), max_workgroups walk and matrix-mode by-products (max |w_new| per row / column, the words cim_amax_rowcol
 * produces) as cim_sgd_multi.  16-byte accesses are used when the four pointers of a tensor are 16-byte aligned. */
typedef struct cim_adam_tensor {
    uint64_t p;            /* float* parameter (device address) */
    uint64_t g;            /* const float* gradient */
    uint64_t exp_avg;      /* float* first moment m (zero-initialised by the caller) */
    uint64_t exp_avg_sq;   /* float* second moment v (zero-initialised by the caller) */
    int64_t n;             /* elements */
    float step_size, bc2_sqrt, wd;
    int32_t rows, cols;    /* matrix mode when cols > 0: see cim_sgd_tensor */
    int32_t reserved;      /* 0 */
    uint64_t row_amax, col_amax;
} cim_adam_tensor;         /* 80 bytes */
int cim_adam_multi(const cim_adam_tensor* tensors, const cim_sgd_chunk* chunks, int n_chunks, double beta1, double beta2, double eps,
                   int max_workgroups, void* stream);

/* Gradient clipping by the global L2 norm (ABI-16 addition: cim_abi_version() stays 16; lib/utils/net.py:15):
 *     norm = sqrt(sum of g^2 over all gradients) ;  coef = max_norm / max(norm, max_norm) ;  g = g * coef
 * with the norm and the coefficient kept on the device.  `grads` and `numel` are DEVICE arrays [n_tensors]: the address and
 * the element count of every (dense, contiguous, fp32) gradient; `chunks` is the fused optimizers' table with flat chunks
 * only (chunk.tensor indexes grads / numel, offsets are multiples of 4 elements, chunk.n is clamped to the tensor's end).
 * 16-byte accesses are used for a tensor whose pointer is 16-byte aligned.  max_workgroups: as cim_sgd_multi.
 * cim_grad_norm_multi: two launches.  The first writes the fp64 sum of squares of every chunk to partial[chunk] (caller's
 *   workspace, every slot written on every call; no atomics, fixed reduction shape), the second sums them in fp64 in an
 *   order that only depends on n_chunks and writes out[0] = (float)norm and out[1] = coef:
 *     NaN when the norm is NaN;  (float)(max_norm / norm), divided in fp64, when norm > max_norm (norm = +inf: 0);  else 1.
 *   The result is bit-identical for every max_workgroups and from run to run.  max_norm >= 0; +infinity = "norm only".
 * cim_grad_scale_multi: one launch behind it on the same stream.  Every workgroup reads out[1]; when it is exactly 1.0f it
 *   returns without touching a gradient, otherwise g = g * out[1] in place (a NaN coefficient makes every gradient NaN).
 * n_chunks == 0: nothing is launched and `out` is left untouched.  No element at or beyond a tensor's end is read or written. */
int cim_grad_norm_multi(const uint64_t* grads, const int64_t* numel, int n_tensors,
                        const cim_sgd_chunk* chunks, int n_chunks, double* partial /* [n_chunks] */,
                        double max_norm, float* out /* [2]: norm, coef */, int max_workgroups, void* stream);
int cim_grad_scale_multi(const uint64_t* grads, const int64_t* numel, int n_tensors,
                         const cim_sgd_chunk* chunks, int n_chunks, const float* out,
                         int max_workgroups, void* stream);

/* ------------------------------------------------------------------ training statistics (ABI-16 addition)
 * The bookkeeping of TrainingStats.UpdateIterStats / GetStats (lib/utils/training_stats.py:65-128,149-167) and of its
 * SmoothedValue (lib/utils/logging.py:60-85) on the device: csrc/train_stats.hip, DESIGN.md 4.17.  Additive:
 * cim_abi_version() stays 16.  `state` is the caller's device buffer of cim_stats_bytes(n_keys, window) bytes, 8-byte
 * aligned, ZERO-FILLED ONCE before the first call, one per tracker; n_keys (tracked scalars per push, the total not
 * counted) and window must be the same in every call on one state.  Calls on different states are independent.
 *
 * cim_stats_push: one single-wave launch.  `values_host` is a HOST array of n_values device addresses of fp32 scalars v_0 ..,
 * read before the call returns: the addresses travel in the kernel arguments (autograd hands out new loss tensors every
 * step; there is no device table to refresh).  All arithmetic is fp32, every operation rounded on its own:
 *   t = ((0 + v_0) + v_1) + ... over the first n_sum values, in argument order (training_stats.py:72-77); the remaining
 *   values (a gradient norm, ...) are tracked and are not part of t.  Columns: the n_values values, then t.
 *   iter_size == 1: every column commits its value.  Otherwise acc = (inner == 0 ? 0 : acc) + x per column, and the call
 *   with inner == iter_size - 1 commits acc / (float)iter_size, IEEE division (:106-128; the total's statistic is the mean
 *   of the per-inner totals).
 *   A commit writes slot (count % window) of the ring [window][n_values + 1], adds to a per-column fp64 running sum,
 *   increments count and, if any committed value is not finite and none was before, records the 1-based commit number.
 * cim_stats_summary: one single-wave launch.  out: float [n_keys + 1][3] = per column (median, last committed value, global
 *   mean = fp64 sum / count rounded to fp32), then int32 [2] = (first non-finite commit or 0, count): 3 (n_keys + 1) + 2
 *   4-byte words.  The median is np.median's over the n = min(count, window) committed values: ascending sort, the middle
 *   element for odd n, (a + b) / 2 in fp32 for even n, NaN when the window holds a NaN or n == 0 (then last and mean are NaN too).
 * Refused before any launch (-1, cim_last_error() names the condition; the state is untouched): n_values / n_keys outside
 * 1..CIM_STATS_MAX_KEYS, n_sum > n_values, window outside 1..CIM_STATS_MAX_WIN, iter_size < 1, inner outside [0, iter_size),
 * a null or misaligned address.  Nothing outside the state's cim_stats_bytes and out's words is read or written. */
#define CIM_STATS_MAX_KEYS 16
#define CIM_STATS_MAX_WIN 64
long long cim_stats_bytes(int n_keys, int window);
int cim_stats_push(const uint64_t* values_host, int n_values, int n_sum, int window, int iter_size, int inner, void* state,
                   void* stream);
int cim_stats_summary(void* state, int n_keys, int window, float* out /* [3 (n_keys + 1) + 2] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIM_HIP_H */
