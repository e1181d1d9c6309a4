/* dynamo_hip.h -- C ABI of libdynamo_hip.so, the MI355X (gfx950) implementation of Dynamo-Depth's
 * per-step view-synthesis loss path.
 *
 * The reference has no FFI: its boundary is the Python operator surface of tools.py / Trainer.py
 * (SURVEY.md section 8(b)).  Each entry point below names the reference code it replaces; the
 * Python side (dynamo-depth_amd/hipops/) binds them with ctypes -- see INTEGRATION.md for the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 NCHW data unless stated otherwise;
 *   - the caller owns all memory (inputs, outputs, workspaces); the library allocates nothing, keeps
 *     no global state and holds no pointer past return;
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*), never synchronise, and
 *     are therefore hipGraph-capturable;
 *   - return value: 0 on success, otherwise a hipError_t (dd_error_string() decodes it);
 *   - "accumulate" outputs are added to (read-modify-write by the single owner of each element; no float atomic is left in
 *     the library, only integer counters) and must be initialised by the caller.
 */
#ifndef DYNAMO_HIP_H_
#define DYNAMO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD_MAX_SCALES 4
#define DD_NUM_SRC 2                 /* source frames (-1, +1); reference options.py frame_ids default */
#define DD_ABI_VERSION 2

/* flow-composition mode = phase flags of Trainer.setup_phase (Trainer.py:466-490) */
#define DD_MODE_RIGID 0              /* disp_init   : bool_CmpFlow=False, bool_MotMask=False */
#define DD_MODE_FLOW 1               /* motion_init : bool_CmpFlow=True,  bool_MotMask=False */
#define DD_MODE_FLOW_MASK 2          /* mask_init / fine_tune : both True                      */

/* per-block partial record written by dd_photo_loss's tile kernel (floats; 30 used, +7 smoothness sums under dd_fused_loss) */
#define DD_PARTIAL_STRIDE 40
/* per-scale sums produced by dd_photo_loss (floats):
 *   [0] sum over B*H*W of the selected photometric loss          (Trainer.py:352 before .mean())
 *   [1],[2] sum over B*3*h*w of valid*(1-mask)*|residual_flow|   per source frame (Trainer.py:386)
 *   [3],[4] sum over B*h*w of disp_mag                           per source frame (Trainer.py:396-397)
 *   [5] number of pixels whose minimum was a warped frame (automask statistics)
 */
#define DD_SUMS_STRIDE 8

typedef struct DDPhotoScale {
  int shift;                         /* scale s: (h,w) = (H>>s, W>>s) */
  int h, w;
  float w_photo;                     /* weight of sums[0] in the differentiated total  */
  float w_cons;                      /* weight of sums[1]+sums[2] in the differentiated total */
  const float* disp;                 /* (B,1,h,w)  outputs[('disp',0,s)] */
  const float* flow[DD_NUM_SRC];     /* (B,3,h,w)  outputs[('complete_flow',f,s)]  (modes 1,2) */
  const float* mask[DD_NUM_SRC];     /* (B,1,h,w)  outputs[('motion_mask',f,s)]    (mode 2)    */
  const float* noise;                /* (B,2,H,W)  tie-break noise of Trainer.py:339, or NULL  */
  /* gradients of the weighted total (NULL when args.want_grad == 0).  Buffers must be zeroed by the caller; at
   * shift == 0 every element is overwritten by its single owner, at shift > 0 contributions are added atomically.
   * The two frames may share one buffer (the reference shares the motion mask between frames): it receives the sum. */
  float* g_disp;                     /* (B,1,h,w) */
  float* g_flow[DD_NUM_SRC];         /* (B,3,h,w) */
  float* g_mask[DD_NUM_SRC];         /* (B,1,h,w) */
  /* optional materialised outputs (NULL = skip) -- the dict entries of SURVEY.md Appendix B */
  float* out_color[DD_NUM_SRC];      /* (B,3,H,W)  outputs[('color',f,s)]                    */
  float* out_sample[DD_NUM_SRC];     /* (B,H,W,2)  outputs[('sample',f,s)]                   */
  float* out_depth;                  /* (B,1,H,W)  outputs[('depth',0,s)]                    */
  float* out_idsel;                  /* (B,H,W)    outputs['identity_selection/s'] (automask) */
  float* out_resid[DD_NUM_SRC];      /* (B,3,h,w)  outputs[('residual_flow',f,s)]  accumulate */
  float* out_delta[DD_NUM_SRC];      /* (B,h,w)    disp_mag of Trainer.py:396      accumulate */
} DDPhotoScale;

typedef struct DDPhotoArgs {
  int abi_version;                   /* DD_ABI_VERSION */
  int B, H, W;
  int num_scales;
  int mode;                          /* DD_MODE_* */
  int automask;                      /* Trainer.bool_automask (Trainer.py:117) */
  int want_grad;
  float min_depth, max_depth;        /* options.py:182-189 */
  float ssim_weight;                 /* options.py:115-118 */
  float eps;                         /* Project3D eps, tools.py:203 */
  float disp_thr;                    /* mask_disp_thrd, options.py:119-122 */
  const float* target;               /* (B,3,H,W) inputs[('color',0,0)] */
  const float* source[DD_NUM_SRC];   /* (B,3,H,W) inputs[('color',f,0)] */
  const float* source_packed[DD_NUM_SRC]; /* optional (NULL, or both set): (B,H,W,3) pixel-interleaved copies of source[f] (dd_pack_rgb) --
                                        same values; the warp gathers one 12-byte pixel per bilinear tap instead of three planes */
  const float* K;                    /* (B,4,4) inputs[('K',0)] */
  const float* inv_K;                /* (B,4,4) inputs[('inv_K',0)] */
  const float* T[DD_NUM_SRC];        /* (B,4,4) outputs[('cam_T_cam',0,f)], last row assumed (0,0,0,1) */
  const float* ts[DD_NUM_SRC];       /* (B,) fp32 inputs[('ts',f)] or NULL (=1) */
  float* g_T[DD_NUM_SRC];            /* (B,4,4) gradient w.r.t. T, overwritten (row 3 = 0); NULL if !want_grad */
  float* sums;                       /* (num_scales, DD_SUMS_STRIDE) overwritten */
  float* workspace;                  /* dd_photo_workspace_bytes() bytes, contents undefined */
  DDPhotoScale scale[DD_MAX_SCALES];
} DDPhotoArgs;

/* Replaces, in one launch pair, Trainer.generate_images_pred (Trainer.py:215-287) + the photometric /
 * automask / c_consistency part of Trainer.compute_losses (Trainer.py:316-352,384-386) + their autograd
 * backward: utils.interp, tools.disp_to_depth (tools.py:291), BackprojectDepth.forward (tools.py:191),
 * Project3D.forward (tools.py:211), F.grid_sample (Trainer.py:281), SSIM.forward (tools.py:243),
 * compute_reprojection_loss (Trainer.py:413). */
int dd_photo_loss(const DDPhotoArgs* args, void* stream);
size_t dd_photo_workspace_bytes(const DDPhotoArgs* args);
/* Measurement aid (bench.py's roofline leg): while enabled, every gradient-carrying dd_photo_loss call that is not under
 * stream capture records a HIP event pair around its photo_tile_kernel launch, on the stream the kernel is launched on
 * (at most 256 pairs between reads).  dd_photo_timing_read waits for the recorded launches, returns their mean duration
 * (ignoring the first `skip`) and forgets them.  Not thread-safe; no reference counterpart. */
int dd_photo_timing(int enable);
int dd_photo_timing_read(float* mean_us, int* launches, int skip);
/* dd_photo_loss in two calls: part 1 launches photo_tile_kernel alone, part 2 the launches that follow it (pyramid combine,
 * finalize); part 0 = dd_photo_loss.  A caller that records the step into hipGraphs can leave part 1 out of the recording and
 * issue it from the host between two graphs (the arguments are fixed addresses), where dd_photo_timing can bracket it with
 * events -- segments.SegmentedStep with time_tile_kernel, used by bench.py's roofline leg.  Same arguments for both parts. */
int dd_photo_loss_part(const DDPhotoArgs* args, void* stream, int part);

/* Edge-aware smoothness, forward + gradient in one pass.  Replaces tools.compute_smooth_loss
 * (tools.py:311-326) and, with normalise=1, the mean-normalisation of Trainer.py:357-359.
 *   inp (B,C,h,w), img (B,3,h,w) or NULL.
 *   sums[0] = sum |dx inp| e^{-mean_c|dx img|}, sums[1] = same in y  (caller divides by the two counts)
 *   g_inp (B,C,h,w) accumulate:  += weight * d( sums[0]/(B*C*h*(w-1)) + sums[1]/(B*C*(h-1)*w) )/d inp,
 *   or NULL.  workspace: dd_smooth_workspace_bytes(B,C,h,w). */
int dd_smooth_loss(const float* inp, const float* img, int B, int C, int h, int w, int normalise, float weight,
                   float* g_inp, float* sums, float* workspace, void* stream);
size_t dd_smooth_workspace_bytes(int B, int C, int h, int w);

/* Above-ground term (Trainer.py:361-364,425-461; tools.GroundPlane tools.py:76-164).
 *   disp (B,1,h,w), inv_K (B,4,4) of this scale, rand_idx (B, max_it*np_per_it) int32 indices into the bottom
 *   int(g_prior*h) rows (the reference draws them with the host NumPy RNG, tools.py:125-127).
 *   out[0] = sum of min(disp - ground_disp, 0) over valid pixels (caller: -out[0]/(B*h*w)/2^s),
 *   plane (B,3) = best plane parameters (before the +tol shift), g_disp (B,1,h,w) accumulate with `weight`
 *   = d(total)/d(out[0]) .  workspace: dd_ground_workspace_bytes(B,h,w,max_it). */
int dd_ground_loss(const float* disp, const float* inv_K, const int32_t* rand_idx, int B, int h, int w,
                   int np_per_it, int max_it, float tol, float g_prior, float min_depth, float max_depth,
                   float weight, float* g_disp, float* plane, float* out, float* workspace, void* stream);
size_t dd_ground_workspace_bytes(int B, int h, int w, int max_it);

/* The two halves of dd_ground_loss separately (parity tests pin each against the reference on its own, tests/test_ground_pin.py):
 * dd_ground_candidates: the least-squares plane of every RANSAC sample (tools.py:141-154 `calc_param`) -> cand (B*max_it,3),
 *   candidate j = b*max_it + it drawn from image b's ground points;
 * dd_ground_select: the reference's decision rule on GIVEN candidates (tools.py:129-137: candidate j scored on image j mod B,
 *   inlier fraction |dist| < tol, first maximum) and everything behind it (Trainer.py:361-364,436-461): counts (B*max_it) inliers
 *   per candidate, plane (B,3), out[0] as dd_ground_loss, g_disp accumulated (may be NULL).  Same workspace. */
int dd_ground_candidates(const float* disp, const float* inv_K, const int32_t* rand_idx, int B, int h, int w, int np_per_it, int max_it,
                         float g_prior, float min_depth, float max_depth, float* cand, void* stream);
int dd_ground_select(const float* disp, const float* inv_K, const float* cand, int B, int h, int w, int max_it, float tol, float g_prior,
                     float min_depth, float max_depth, float weight, float* g_disp, int32_t* counts, float* plane, float* out,
                     float* workspace, void* stream);

/* tools.GroundPlane.forward (tools.py:85-101) on an explicit point map: points (B,3,h,w) ->
 * dist (B,1,h,w) vertical distance to the best RANSAC plane, plane (B,3).  Same workspace size as above. */
int dd_ground_plane(const float* points, const int32_t* rand_idx, int B, int h, int w, int np_per_it, int max_it,
                    float tol, float g_prior, float* dist, float* plane, float* workspace, void* stream);

/* Folds the raw sums written by the kernels above into the `losses` dict values of Trainer.compute_losses
 * (Trainer.py:404-409) in one tiny launch (no host round trip, weights are launch-time scalars):
 *   term[s][t] = sum_i [scale_of[i]==s && term_of[i]==t] * norm[i] * res[i]
 *   out[1+t]   = sum_s term[s][t]                    ('loss_term/<name>')
 *   out[8+s]   = sum_t coef[t] * term[s][t]          ('loss_term/<s>')
 *   loss[0]    = sum_s out[8+s] / num_scales         ('loss')          out[0] = loss[0] as well
 * res entries with term_of[i] < 0 are ignored. */
#define DD_NUM_TERMS 7
#define DD_MAX_RES 128
typedef struct DDAssembleArgs {
  int n;                              /* entries of res */
  int num_scales;
  float coef[DD_NUM_TERMS];           /* losses['loss_coef/<name>'] in options.py g_* order */
  float norm[DD_MAX_RES];
  int8_t term_of[DD_MAX_RES];
  int8_t scale_of[DD_MAX_RES];
} DDAssembleArgs;
int dd_assemble_losses(const float* res, const DDAssembleArgs* args, float* loss, float* out, void* stream);

/* All regularisers of Trainer.compute_losses for every scale in a handful of launches (the per-term entry points above take two to
 * four launches per term and scale -- about 45 per step at three scales); the smoothness of ALL smoothed tensors of a scale is
 * one pass that forms the edge weights once per pixel: edge-aware smoothness of disp / flow / mask
 * (tools.py:311-326, Trainer.py:355-359,380-381,401-402), mask sparsity (Trainer.py:393-399), ground term (Trainer.py:361-364,
 * 425-461).  Same per-element arithmetic as dd_smooth_loss / dd_ground_loss; the smoothness sums are folded
 * per entry instead of per channel (a different, equally fixed order: the last bits of the value may differ from dd_smooth_loss).
 * A `smooth` entry with inp == NULL is skipped; the caller merges entries whose tensors are shared between the two frames
 * (weight = sum of the frames' weights).  A sparsity entry with prob == NULL and a ground entry with disp == NULL are skipped.
 * Raw sums go to res[scale * DD_REG_RES_STRIDE + slot]:
 *   slot 2*k, 2*k+1 (k < DD_REG_SMOOTH): smooth entry k -> sum |dx| e^-|dx img|, sum |dy| e^-|dy img|
 *   slot 10 + 2*f, 11 + 2*f           : sparsity frame f -> loss value (mean over static pixels, 0 if gated off), #static
 *   slot 14                            : ground -> sum of min(disp - ground_disp, 0)
 * Gradients are accumulated into the g_* buffers with the given weights, exactly like the per-term entry points. */
#define DD_REG_SMOOTH 5
#define DD_REG_RES_STRIDE 16
typedef struct DDRegSmooth {
  const float* inp;                  /* (B,C,h,w) */
  float* g_inp;                      /* accumulate, or NULL */
  int C;
  int normalise;                     /* 1: divide by the per-image mean first (disparity, C == 1) */
  float weight;                      /* d(total)/d(mean_x + mean_y) */
} DDRegSmooth;
typedef struct DDRegScale {
  int h, w;
  const float* img;                  /* (B,3,h,w) target pyramid level */
  DDRegSmooth smooth[DD_REG_SMOOTH];
  const float* delta[DD_NUM_SRC];    /* (B,h,w) disp_mag from dd_photo_loss */
  const float* delta_sum[DD_NUM_SRC];/* device scalar: its sum over the batch */
  const float* prob[DD_NUM_SRC];     /* (B,1,h,w) motion_prob, NULL = no sparsity term for this frame */
  float* g_prob[DD_NUM_SRC];
  float w_sparsity[DD_NUM_SRC];
  const float* disp;                 /* ground term: (B,1,h,w), NULL = off */
  float* g_disp;
  const float* inv_K;                /* (B,4,4) of this scale */
  const int32_t* rand_idx;           /* (B, max_it*np_per_it) */
  float* plane;                      /* (B,3) out */
  float w_ground;
} DDRegScale;
typedef struct DDRegArgs {
  int abi_version;
  int B, num_scales;
  int np_per_it, max_it;             /* RANSAC (options.py:198-213) */
  float tol, g_prior, min_depth, max_depth;
  float* res;                        /* (num_scales, DD_REG_RES_STRIDE), zeroed by the caller; the slots of active terms are overwritten */
  float* workspace;                  /* dd_reg_workspace_bytes() bytes */
  DDRegScale scale[DD_MAX_SCALES];
} DDRegArgs;
size_t dd_reg_workspace_bytes(const DDRegArgs* args);
/* The regularisers above followed by dd_assemble_losses on the same `res` record (args->res; the caller's photometric sums already
 * sit behind the regulariser slots): the fold of the ground-hinge partials runs inside the assembling kernel.  Four stage launches
 * (plus one each for the quad smoothness and the candidate scoring) for the regularisers of all scales + one for the loss assembly
 * (reference Trainer.py:355-409). */
int dd_reg_losses_finish(const DDRegArgs* args, const DDAssembleArgs* assemble, float* loss, float* out, void* stream);

/* THE fused loss: dd_photo_loss + dd_reg_losses_finish on the same arguments in FIVE launches instead of ten (round 5) -- the whole of
 * Trainer.generate_images_pred + Trainer.compute_losses and their backward (Trainer.py:215-411, tools.py:76-164,191-257,291-326):
 *   1  the photometric tile kernel; at scale 0 the edge-aware smoothness of the disparity / flow / mask (tools.py:311-326,
 *      Trainer.py:355-359,380-381,401-402) is evaluated in its store stage and added to the pixel's gradient before its one store;
 *      extra workgroups of the same launch solve the RANSAC candidates (tools.py:114-154) and take the per-image disparity sums;
 *   2  one launch of tasks: low-res gradient footprints summed AND the smoothness of the scales >= 1 in the same pass | fold of the
 *      tile records | inlier counts of the candidates;
 *   3  static-pixel counts (Trainer.py:393-399) | per-image scalars: smoothness sums, mean, winning plane;
 *   4  sparsity gradient | mean-normalisation adjoint + ground hinge (Trainer.py:361-364,425-461);
 *   5  the losses dict values (Trainer.py:404-409).
 * `photo` and `reg` are filled exactly as for the two calls they replace (same workspaces: dd_photo_workspace_bytes /
 * dd_reg_workspace_bytes; photo->sums behind the regulariser slots of reg->res as dd_reg_losses_finish expects).  The request takes
 * this pipeline when it is a gradient pass whose two frames share their flow / mask tensors (or the rigid mode), every smoothness
 * entry is one of the photometric tensors (disparity, mean-normalised | flow | mask) accumulating into the photometric gradient
 * buffer, the scale-0 pyramid level is the target image and the rows of the scales >= 1 are whole 16-byte aligned quads --
 * dd_fused_loss_supported says so (0: no; 1: yes; 2: yes, and every element of every gradient buffer named in the two argument blocks
 * is written by exactly one plain store, so the caller need not zero them first -- motion_prob's gradient included, which under the
 * other entry points is an accumulate-type output); dd_fused_loss returns hipErrorNotSupported (801) otherwise and launches nothing:
 * the caller then issues dd_photo_loss + dd_reg_losses_finish.  The disparity smoothness is evaluated on the raw disparity and divided
 * by (mean + eps) per image afterwards (the reference divides first: equal up to rounding); gradients of one element are written
 * once (no read-modify-write of the flow / mask planes).  dd_fused_loss_part: 1 = the tile kernel alone, 2 = the launches behind it
 * (see dd_photo_loss_part). */
int dd_fused_loss(const DDPhotoArgs* photo, const DDRegArgs* reg, const DDAssembleArgs* assemble, float* loss, float* out, void* stream);
int dd_fused_loss_part(const DDPhotoArgs* photo, const DDRegArgs* reg, const DDAssembleArgs* assemble, float* loss, float* out, void* stream,
                       int part);
int dd_fused_loss_supported(const DDPhotoArgs* photo, const DDRegArgs* reg);

/* ---- baseline JPEG decoding of a batch of frames (csrc/dd_jpeg.hip; SURVEY.md 8(f) row 1, first stage) ------------------------
 * Replaces datasets/base_dataset.py:13-18 `pil_loader` (PIL / libjpeg decode of the three frames of every sample in the DataLoader
 * workers, base_dataset.py:140-147) for files that are already at the training resolution -- the reference's `downsample` image
 * type.  The result is PIL's, bit for bit: sequential Huffman decoding, ISLOW integer IDCT, "fancy" triangle chroma up-sampling,
 * 16-bit fixed-point YCbCr -> RGB.
 * One header record per image, filled on the host from the marker segments (hipops/jpeg.py parse_header): */
typedef struct DDJpegHeader {
  int32_t data_offset;               /* first byte of the entropy-coded segment, relative to the image's first byte */
  int32_t data_end;                  /* file length */
  int32_t width, height;
  int32_t restart_interval;          /* MCUs between RSTn markers, 0 = none */
  int32_t ncomp;
  int32_t h[3], v[3], tq[3], td[3], ta[3];
  int32_t reserved[3];               /* qt at byte 96: the kernels read the tables 16 bytes at a time; sizeof = 1696 = 106 x 16 */
  uint16_t qt[4][64];                /* quantisation tables, natural (de-zigzagged) order */
  uint8_t bits[4][16];               /* Huffman tables dc0, dc1, ac0, ac1: number of codes per length ... */
  uint8_t vals[4][256];              /* ... and the symbols in code order (T.81 B.2.4.2) */
} DDJpegHeader;
/* data: image i occupies data[i*stride, i*stride + headers[i].data_end); all images H x W with `ncomp` components of sampling (h,v)
 * (luma 1x1 / 2x1 / 1x2 / 2x2, chroma 1x1).  rgb: (n_images, H, W, 3) uint8, what dd_prepare_frames reads.  Three launches. */
size_t dd_jpeg_workspace_bytes(int n_images, int H, int W, int ncomp, const int* h, const int* v);
int dd_jpeg_decode(const unsigned char* data, long long stride, const DDJpegHeader* headers, int n_images, int H, int W, int ncomp, const int* h,
                   const int* v, unsigned char* rgb, void* workspace, size_t workspace_bytes, void* stream);

/* transforms.Resize((H, W), BICUBIC) on PIL frames (datasets/base_dataset.py:80,147) = Pillow's Image.resize, on the device, bit for
 * bit: src (n_images, Hs, Ws, 3) uint8 -> dst (slots, H, W, 3) uint8, image i written to slot dst_slot[i] (NULL: slot i).  The tap
 * tables are Pillow's precompute_coeffs + normalize_coeffs_8bpc (hipops/resize.py builds them): *_bounds (out, 2) = first input
 * index and tap count per output index, *_coef (out, ksize) 22-bit fixed-point weights; the tables of an axis whose size does not
 * change may be NULL (Pillow skips that pass).  workspace: dd_resize_workspace_bytes (the horizontal pass's output). */
size_t dd_resize_workspace_bytes(int n_images, int Hs, int Ws, int H, int W);
int dd_resize_bicubic(const unsigned char* src, int n_images, int Hs, int Ws, unsigned char* dst, const int32_t* dst_slot, int H, int W,
                      const int32_t* h_bounds, const int32_t* h_coef, int h_ksize, const int32_t* v_bounds, const int32_t* v_coef, int v_ksize,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Area-weighted down-sample, OpenCV's INTER_AREA for any down-scale (reference prepare_data/nuScenes.py:152, 1600x900 -> 512x288):
 * src (n,Hs,Ws,3) uint8, 16-byte aligned -> dst (n,Hd,Wd,3) uint8 with Hd <= Hs and Wd <= Ws.  Per axis the host builds
 * (hipops/resize.py area_table): start [D] int32 first source index, count [D] int32 taps, weight (D,taps) float32 padded with
 * zeros.  dst = the separable weighted sum, columns first, then rows, in fp32 with one fused multiply-add per tap in ascending tap
 * order, rounded half to even, saturated; DESIGN 4.22.  One launch; source rows staged through LDS, no atomics, no workspace.
 * hipErrorInvalidValue (1): a NULL pointer, a non-positive size, an up-scale, more than 65535 images, taps above 1024, Hs*Ws*3 above
 * 2^31-1, a scale so large that one destination column's strip does not fit the staging buffer, a misaligned src. */
int dd_resize_area(const unsigned char* src, int n_images, int Hs, int Ws, unsigned char* dst, int Hd, int Wd, const int32_t* h_start,
                   const int32_t* h_count, const float* h_weight, int h_taps, const int32_t* v_start, const int32_t* v_count,
                   const float* v_weight, int v_taps, void* stream);

/* ---- operator-level entry points: the tools.py modules one by one (forward; *_bwd = autograd) ---- */

/* tools.BackprojectDepth.forward (tools.py:191-197): depth (B,1,h,w), inv_K (B,4,4) -> points (B,4,h*w) */
int dd_backproject(const float* depth, const float* inv_K, int B, int h, int w, float* points, void* stream);
int dd_backproject_bwd(const float* g_points, const float* inv_K, int B, int h, int w, float* g_depth, void* stream);

/* tools.Project3D.forward (tools.py:211-224): points (B,4,N), K (B,4,4), T (B,4,4) or NULL ->
 * pix (B,h,w,2) normalised to [-1,1], ego (B,3,N) */
int dd_project3d(const float* points, const float* K, const float* T, int B, int h, int w, float eps,
                 float* pix, float* ego, void* stream);
/* g_points (B,4,N) overwritten; g_T (B,4,4) overwritten (NULL when T is NULL); workspace B*nblocks*16 floats
 * (dd_project3d_workspace_bytes; nblocks = ceil(h*w / 256)).  g_pix or g_ego may be NULL: that output's upstream gradient is 0. */
int dd_project3d_bwd(const float* points, const float* K, const float* T, const float* g_pix, const float* g_ego,
                     int B, int h, int w, float eps, float* g_points, float* g_T, float* workspace, void* stream);
size_t dd_project3d_workspace_bytes(int B, int h, int w);

/* tools.SSIM.forward (tools.py:243-257): x, y (B,C,H,W) -> (B,C,H,W);  *_bwd: g_x, g_y overwritten (either may be NULL) */
int dd_ssim(const float* x, const float* y, int B, int C, int H, int W, float* out, void* stream);
int dd_ssim_bwd(const float* x, const float* y, const float* g_out, int B, int C, int H, int W,
                float* g_x, float* g_y, void* stream);

/* tools.disp_to_depth (tools.py:291-298) elementwise over n values */
int dd_disp_to_depth(const float* disp, size_t n, float min_depth, float max_depth, float* scaled, float* depth,
                     void* stream);

/* networks.layers.transformation_from_parameters (networks/layers.py:7-82): axisangle, translation (B,3) -> (B,4,4) */
int dd_pose_matrix(const float* axisangle, const float* translation, int B, int invert, float* T, void* stream);
int dd_pose_matrix_bwd(const float* axisangle, const float* translation, const float* g_T, int B, int invert,
                       float* g_axisangle, float* g_translation, void* stream);

/* Element-typed entry points (the `_t` suffix): `dtype` selects the type of the activation / gradient tensors passed as void* --
 * DD_DTYPE_F32, DD_DTYPE_F16, DD_DTYPE_BF16; the last two are the tensors of an autocast forward (config "fp16 convs" of BASELINE.json,
 * config 5 with the LiteMono depth net) -- read and written four elements at a time (half types move 8 bytes per access).  Statistics,
 * affine parameters, convolution weights (the fp32 master copies), sums and every intermediate stay fp32. */
#define DD_DTYPE_F32 0
#define DD_DTYPE_F16 1
#define DD_DTYPE_BF16 2

/* Bias gradient of a convolution whose output gradient is channels-last: out[c] = sum over rows of x[row*C + c]
 * (x = (B,H,W,C) memory of type `dtype`, rows = B*H*W; out fp32).  Replaces ATen's generic reduction, which is ~100x off the HBM roofline for
 * small C (the full-resolution 9-channel convs of networks/motion_decoder.py); any C >= 1 (C > 256, the bias gradients of
 * LiteMono's point-wise Linears -- networks/depth_encoder.py:200-203 --, takes a column-per-thread kernel).
 * workspace: dd_channel_sum_workspace_bytes(C). */
int dd_channel_sum_nhwc_t(const void* x, long long rows, int C, float* out, int dtype, float* workspace, void* stream);
size_t dd_channel_sum_workspace_bytes(int C);

/* nn.ReflectionPad2d(1) of networks.layers.Conv3x3 (reference networks/layers.py:100-115) for channels-last tensors:
 * x (B,H,W,C) memory -> out (B,H+2,W+2,C); *_bwd is its adjoint (g_out (B,H+2,W+2,C) -> g_x (B,H,W,C), overwritten). */
int dd_reflect_pad1_nhwc_t(const void* x, int B, int H, int W, int C, void* out, int dtype, void* stream);
int dd_reflect_pad1_nhwc_bwd_t(const void* g_out, int B, int H, int W, int C, void* g_x, int dtype, void* stream);

/* Depth-wise (groups == channels) 3x3 convolution, stride 1, zero padding == dilation, no bias, on channels-last tensors:
 * LiteMono's CDilated inside DilatedConv (reference networks/depth_encoder.py:168-181, 197-199 -- nn.Conv2d(dim, dim, 3,
 * padding=d, dilation=d, groups=dim, bias=False)). x, out, g_*: [B,H,W,C] elements of type `dtype` (the memory of a channels_last NCHW
 * tensor), weight/g_weight: [C,1,3,3] contiguous fp32; C a multiple of 4, <= 512. The weight gradient is a fixed-order two-level sum
 * (one record per image row in `workspace`, dd_dwconv3x3_workspace_bytes(B,H,C) bytes), so it is run-to-run reproducible. */
int dd_dwconv3x3_nhwc_t(const void* x, const float* weight, int B, int H, int W, int C, int dilation, void* out, int dtype, void* stream);
int dd_dwconv3x3_nhwc_bwd_data_t(const void* g_out, const float* weight, int B, int H, int W, int C, int dilation, void* g_x, int dtype, void* stream);
int dd_dwconv3x3_nhwc_bwd_weight_t(const void* g_out, const void* x, int B, int H, int W, int C, int dilation, float* g_weight, void* workspace,
                                   size_t workspace_bytes, int dtype, void* stream);
size_t dd_dwconv3x3_workspace_bytes(int B, int H, int C);

/* Data gradient of a 3x3, stride-1 convolution with ONE output channel (the disparity heads: networks/depth_decoder.py:49-51,
 * 95-97, `Conv3x3(num_ch_dec[s], 1)`): g_out [B,Ho,Wo] (one channel), weight [1,C,3,3], g_x [B,Hi,Wi,C] channels-last,
 * Ho = Hi + 2*padding - 2, padding 0 (input already reflection-padded) or 1.  C a multiple of 4, <= 512. */
int dd_conv3x3_cout1_bwd_data(const float* g_out, const float* weight, int B, int Hi, int Wi, int C, int padding, float* g_x, void* stream);

/* Input side of a training step on the device.  The reference prepares every sample on the host in the
 * DataLoader workers: ToTensor, torchvision ColorJitter on the float tensor of each frame (a fresh draw per frame,
 * datasets/base_dataset.py:83-95,159-164), horizontal flip (:118-131); Trainer.apply_img_resize then builds the target pyramid
 * (Trainer.py:722-734).  Here the loader hands over the decoded uint8 frames and the drawn parameters.
 *   frames_u8 (B,F,H,W,3) uint8 RGB;  params (B,F,9) fp32 rows [apply, fn_idx[4] (0 brightness 1 contrast 2 saturation 3 hue),
 *   brightness, contrast, saturation, hue];  flip (B) int32.
 *   color, color_aug (F,B,3,H,W) fp32 in [0,1]: ('color',f,0) and ('color_aug',f,0) of frame f = one contiguous (B,3,H,W) block.
 * workspace: dd_prepare_frames_workspace_bytes(B,F).  Two launches. */
int dd_prepare_frames(const uint8_t* frames_u8, const float* params, const int32_t* flip, int B, int F, int H, int W, float* color,
                      float* color_aug, float* workspace, void* stream);
size_t dd_prepare_frames_workspace_bytes(int B, int F);
/* One pyramid level: dst = clamp(F.interpolate(src, (H/2,W/2), 'bicubic', align_corners=False, antialias=True), 0, 1) -- the tensor
 * Resize(BICUBIC) of Trainer.py:80 as ATen computes it (Keys cubic a = -0.5, support widened by the scale, border taps
 * renormalised, horizontal then vertical).  src (planes,H,W), dst (planes,H/2,W/2); H, W even. */
int dd_pyramid_down2(const float* src, int planes, int H, int W, float* dst, void* stream);
/* (B,3,H,W) planar fp32 -> (B,H,W,3) pixel-interleaved fp32, same values: the layout DDPhotoArgs.source_packed takes.  The
 * reference has no counterpart (F.grid_sample reads the planar tensor, Trainer.py:281); the input side issues it once per step
 * for the two source frames, the photometric kernel then gathers from it at every scale.  H*W must be a multiple of 4. */
int dd_pack_rgb(const float* planar, int B, int H, int W, float* packed, void* stream);

/* tools.DepthMetrics.forward without a mask (tools.py:16-73) and compute_errors (tools.py:269-288): sparse-LiDAR depth
 * metrics with per-image median scaling -- SURVEY.md 8(f) row 2, the accuracy gate of the evaluation.
 * disp [B,1,H,W] (outputs['disp_scaled',0,0]); lidar [B,M,3] = (row, col, depth) in ground-truth pixels, padded;
 * valid [B,M] floats (0 = padding); gt_dim [B,2] int32 (height, width) on the DEVICE; img_bound: 4 doubles on the HOST
 * (opt.eval_img_bound: up, down, left, right fractions). per_sample [B,8] = abs_rel, sq_rel, rms, log_rms, a1, a2, a3,
 * kept-point count; mean [7] = batch mean as the reference returns it. A sample with no kept point yields NaNs (the
 * reference raises). workspace: dd_depth_metrics_workspace_bytes(B, M). One workgroup per sample, no host sync.
 * Workspace layout (what the kernel leaves there): per sample M floats of ground truth, M floats of predicted depth, and in the
 * masked call M int32 labels. Dropped points carry -1 in the first two (their label slot is not written).
 * hipErrorInvalidValue, nothing launched: a NULL pointer, B, H, W or M < 1 (masked: mask_h or mask_w < 1), a workspace too small. */
int dd_depth_metrics(const float* disp, int B, int H, int W, const float* lidar, const float* valid, int M, const int* gt_dim,
                     const double* img_bound, float min_depth, float max_depth, float* per_sample, float* mean,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t dd_depth_metrics_workspace_bytes(int B, int M);
/* The mask branch of tools.DepthMetrics.forward (tools.py:23-25,58-72): `mask` (B,mask_h,mask_w) uint8 labels in ground-truth pixels
 * (the loaders' sem_mask / mot_mask).  per_label [B,256,8] = for every label that occurs among a sample's kept LiDAR points, the seven
 * errors over those points and their count (zero rows otherwise); the caller forms sum_b err*cnt and sum_b cnt per label.
 * A mask smaller than the ground truth: a point outside it carries label 0.
 * workspace: dd_depth_metrics_masked_workspace_bytes(B, M), laid out as above with the labels as the third block of every sample. */
int dd_depth_metrics_masked(const float* disp, int B, int H, int W, const float* lidar, const float* valid, int M, const int* gt_dim,
                            const double* img_bound, float min_depth, float max_depth, const uint8_t* mask, int mask_h, int mask_w,
                            float* per_sample, float* mean, float* per_label, void* workspace, size_t workspace_bytes, void* stream);
size_t dd_depth_metrics_masked_workspace_bytes(int B, int M);
/* Cross-batch totals of a depth evaluation, kept on the device (the reference's eval/depth.py pulls seven scalars to the host per batch).
 * per_sample [B,8] as dd_depth_metrics writes it; per_label [B,256,8] as dd_depth_metrics_masked writes it, or NULL.
 * totals [9] doubles, ACCUMULATED into: [0..6] += (double)per_sample[b][j] over the samples with per_sample[b][7] > 0, in batch order;
 * [7] += the number of such samples; [8] += the number of samples without a kept LiDAR point (their NaN rows are not summed).
 * label_totals [256,8] doubles, ACCUMULATED into (NULL iff per_label is NULL): [l][j<7] += (double)per_label[b][l][j] * (double)per_label[b][l][7],
 * [l][7] += per_label[b][l][7], in batch order.  The caller zeroes both once per evaluation (as dd_motion_pr's counts).
 * One workgroup of 256 threads, every slot summed by one thread: no atomics, no reduction across threads -- the totals are identical
 * from run to run and independent of how the dataset is cut into batches.
 * hipErrorInvalidValue, nothing launched: per_sample or totals NULL, B < 1, exactly one of per_label / label_totals NULL. */
int dd_depth_metrics_accumulate(const float* per_sample, const float* per_label, int B, double* totals, double* label_totals, void* stream);

/* The reference's odometry evaluation behind the network (eval/odometry.py:19-41,70-96), in float64 on the device.
 * pred (N,4,4) fp32: transformation_from_parameters(axisangle, translation) of the frame pairs (0 -> +1), widened on load;
 * gt_global (N+1,4,4) float64 global camera poses, affine (last row 0 0 0 1).
 * Snippet i = 0 .. S-1 has P = min(track_length-1, N-i) + 1 points: the translations of the running product I.T_i.T_{i+1}... with the
 * axes reordered (z, x, y), against the same running product over the local poses inv(inv(G[k-1]).G[k]).
 * ate[i] = sqrt(sum |scale.pred - gt|^2) / P after aligning the first points, scale = sum(gt.pred) / sum(pred^2), unguarded: an all-zero
 * prediction gives NaN as in the reference.  speed[i] = mean distance between consecutive ground-truth points.
 * A snippet is kept iff P >= track_length - 1, so S = dd_odom_snippet_count(N, track_length) = max(0, min(N, N - track_length + 3)) and
 * the LAST kept snippet is one point shorter than the others (the reference's behaviour, reproduced).
 * One thread per snippet; S == 0 returns success without a launch.  hipErrorInvalidValue (dd_odom_snippet_count: -1) for
 * track_length outside [2, 16] or N < 1; hipErrorInvalidValue for a NULL pointer with S > 0. */
int dd_odom_snippet_count(int N, int track_length);
int dd_odom_snippets(const float* pred, const double* gt_global, int N, int track_length, double* ate, double* speed, void* stream);

/* Motion-segmentation precision/recall counts in one pass (reference eval/motion_segmentation.py:52-95,118-140: the
 * (B, T, H, W) `pred_mask > thrds` scan with its three sums per sample, and the second walk over the dataset for the
 * false-positive tally).  pred [B,1,h,w] (outputs['motion_mask',-1,0]); mot, sem [B,H,W] uint8 labels in ground-truth pixels
 * (mot: 1 = moving, 2 = static, 3 = unlabelled); thresholds [T] on the DEVICE.
 * counts: (2 + num_sem, T + 1) uint64, ACCUMULATED into (caller zeroes once per evaluation).
 * bin(p) = #{k : up(pred)(p) > thresholds[k]}   (strict; NaN -> bin 0), thresholds ascending, 1 <= T <= 256;
 *          up() = F.interpolate(mode='bilinear', align_corners=False) from (h,w) to (H,W) in fp32 (a copy at equal sizes, as in ATen)
 * row 0: pixels with mot == 1              by bin
 * row 1: pixels with mot != 3              by bin
 * row 2+l (l < num_sem <= 32): pixels with mot != 1 && mot != 3 && sem == l, by bin (sem may be NULL iff num_sem == 0;
 *         labels >= num_sem are counted in no row)
 * tp[k] / p_sum[k] of the reference = sum over bins > k of row 0 / row 1; false positives of class l at threshold k = the same
 * sum of row 2+l.  Integer atomics only: the counts are exact and identical from run to run.  hipErrorInvalidValue for T or
 * num_sem out of range, or sem == NULL with num_sem > 0. */
int dd_motion_pr(const float* pred, int B, int h, int w, const uint8_t* mot, const uint8_t* sem, int H, int W,
                 const float* thresholds, int T, int num_sem, unsigned long long* counts, void* stream);

/* Motion masks from per-object contour lists (reference datasets/waymo_dataset.py:109-118: cv2.drawContours(..., -1, label, -1) per
 * object): the exact integer fill of closed contours whose segments are horizontal, vertical or 45 degree diagonals (what
 * cv2.findContours(CHAIN_APPROX_SIMPLE) emits) -- edge pixels and the even-odd interior over all contours of an object (half-open
 * crossing rule: a segment counts on rows min(y0,y1) <= y < max(y0,y1)), the last object in file order wins; DESIGN 4.15.
 * vertices (B,v_cap,2) int16 [x,y]; contours (B,c_cap,6) int32 records [first vertex, vertex count, object index, label 1..255,
 * first row, last row], used records first and in file order (the contours of one object adjacent), a count of 0 ends the list;
 * hipops/contours.py `pack` writes and validates them.  mask (B,H,W) uint8: every byte is written, by one launch, integers only.
 * hipErrorInvalidValue for NULL pointers, non-positive sizes, H or W above 32768 (int16 vertices), B above 65535. */
int dd_fill_contours(const int16_t* vertices, int v_cap, const int32_t* contours, int c_cap, int B, int H, int W, uint8_t* mask,
                     void* stream);

/* KITTI LiDAR depth lists (reference prepare_data/kitti.py:104-115 with kitti_util.py generate_depth_map(..., vel_depth=True)): every
 * scan of a batch projected through every camera matrix, z-buffered with the reference's duplicate rule, and the positive pixels
 * written as row-major [r, c, d] rows; DESIGN 4.18 holds the definition, hipops/lidar.py depth_points_host restates it in numpy.
 * points (n_total,4) float32, 16-byte aligned, column 3 ignored: scan s is rows offsets[s] .. offsets[s+1]-1.
 * offsets [S+1] int32 on the HOST (read and validated before anything is launched, not held past return): offsets[0] == 0,
 *   non-decreasing, offsets[S] == n_total.
 * P (C,3,4) float64 on the device, one matrix per camera, shared by the batch.  Job (s,c) = scan s through P[c], an H x W image.
 * counts [S*C] int32: counts[s*C+c] = rows of job (s,c); every count is written.
 * rows (C*n_total,3) float64: job (s,c) owns the rows C*offsets[s] + c*n_s .. + n_s - 1 (n_s = offsets[s+1]-offsets[s]) and writes the
 *   first counts[s*C+c] of them (a job has at most one row per point); the rest of its segment is left as it was.
 * maps NULL or (S,C,H,W) float32: the dense map of every job, every element written.
 * workspace: dd_lidar_depth_points_workspace_bytes(S, C, H, W), 4-byte aligned; initialised on the stream by the call.
 * Integer min/max atomics only: every output byte is the same from run to run.  4 launches and one memset per 16 scans.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer (maps excepted), S < 1, C < 1 or > 65535, H < 1, W < 2, H*W or n_total
 * above 2^31-1, offsets that decrease or do not run from 0 to n_total, a workspace that is too small, a misaligned pointer. */
size_t dd_lidar_depth_points_workspace_bytes(int S, int C, int H, int W);
int dd_lidar_depth_points(const float* points, long long n_total, const int32_t* offsets, int S, const double* P, int C, int H, int W,
                          int32_t* counts, double* rows, float* maps, void* workspace, size_t workspace_bytes, void* stream);

/* nuScenes LiDAR lists (reference prepare_data/nuScenes.py:157-198): every point of a batch of scans carried sensor -> ego (lidar
 * time) -> global -> ego (camera time) -> camera by four rigid steps applied one after the other in float64 (unfused, each dot
 * product left to right), projected with the 3x3 intrinsics and kept where depth > 1, 1 < u < W-1, 1 < v < H-1; DESIGN 4.22,
 * hipops/lidar.py pose_points_host restates it in numpy.
 * points (n_total,4) float32, 16-byte aligned, column 3 ignored; offsets [S+1] int32 on the HOST as for dd_lidar_depth_points.
 * params (S,64) float64 on the device, per scan: R1[9] t1[3] R2[9] t2[3] t3[3] R3[9] t4[3] R4[9] K[9] W H and 5 unused words, row-major
 *   matrices as they are applied: p = R1 p + t1; p = R2 p + t2 (the global point); p = R3 (p - t3); p = R4 (p - t4); a = K p.
 * counts [S] int32: kept points per scan, every one written.
 * rows (n_total,6) float64 [u, v, depth, gx, gy, gz]: scan s writes the first counts[s] rows from row offsets[s], in scan order;
 *   the rest of its segment is left as it was.
 * workspace: dd_lidar_pose_points_workspace_bytes(S, longest scan), 4-byte aligned.  3 launches per 16 scans, no atomics.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer, S < 1, n_total negative or above 2^31-257, bad offsets, a workspace that
 * is too small, a misaligned pointer. */
size_t dd_lidar_pose_points_workspace_bytes(int S, long long n_max);
int dd_lidar_pose_points(const float* points, long long n_total, const int32_t* offsets, int S, const double* params, int32_t* counts,
                         double* rows, void* workspace, size_t workspace_bytes, void* stream);

/* Motion labels of a nuScenes key frame (reference prepare_data/nuScenes.py:209-244, get_intersect_fraction): per movable panoptic
 * label the number of its points strictly inside every annotation box of its category, and the first box with the strictly
 * greatest count; hipops/lidar.py box_fit_host restates it.  All pointers on the device.
 * points (n_points,3) float64, the points of label l contiguous: rows seg[l] .. seg[l+1]-1 (seg [L+1] int32, clamped to n_points).
 * label_cat [L], box_cat [B] int32 category indices.  boxes (B,16) float64: p1[3], i = p2-p1, j = p4-p1, k = p5-p1, i.i, j.j, k.k,
 *   one unused word; a point p is inside where 0 < (p-p1).i < i.i and the same for j and k, sums left to right, unfused.
 * counts (L,B) int32: points of l inside b, -1 where the categories differ.  best (L,2) int32: [box, count], box -1 and count 0
 *   where no box of the category holds a point.  One launch, integer sums in a fixed order; L == 0 launches nothing.
 * hipErrorInvalidValue (1): negative sizes, L*B above 2^31-1, a NULL pointer that would be read or written, a misaligned pointer. */
int dd_box_fit(const double* points, int n_points, const int32_t* seg, const int32_t* label_cat, int L, const double* boxes,
               const int32_t* box_cat, int B, int32_t* counts, int32_t* best, void* stream);

/* Waymo range images to vehicle-frame points and one camera's depth list (reference prepare_data/waymo.py:183-186, 213-241);
 * DESIGN 4.23, hipops/lidar.py range_image_points_host restates it in numpy.  S images, image s of H_s x W_s pixels.
 * range [n_total] float32 (first return, channel 0) and cp (n_total,3) int32 (the first camera projection [camera, x, y]), image s
 *   from pixel desc[s][0] on, row-major.  pose (n_pose,6) float32 (roll, pitch, yaw, x, y, z) for the images that carry a per-pixel
 *   pose, NULL when n_pose is 0.  trig [n_trig] float64, per image cos incl [H], sin incl [H], cos az [W], sin az [W], built on the host.
 * desc (S,5) int32 on the HOST: first pixel, H, W, first pose pixel or -1, first trig word; the images' pixel ranges ascend and do
 *   not overlap.
 * params (S,64) float64 on the device, per image: E_R[9] E_t[3], one unused word, F_R[9] F_t[3] (inverse frame pose, used with a
 *   pose), C_R[9] C_t[3] (vehicle to camera), K[9], width, height, 16 unused words; row-major, p' = R p + t.
 *   p = rho (cos az cos incl, sin az cos incl, sin incl); p = E p; with a pose p = Rz(yaw) Ry(pitch) Rx(roll) p + (x, y, z), p = F p;
 *   valid where rho > 0.  a = K (C p); kept where a_z > 0, 0 <= a_x/a_z < width, 0 <= a_y/a_z < height.  float64, unfused.
 * counts (S,2) int32 [valid, kept].  points (n_total,3) float64, cp_out (n_total,3) int32: image s writes its valid pixels in
 *   row-major order from row desc[s][0]; rows (n_total,3) float64 [a_x/a_z, a_y/a_z, a_z] of its kept pixels likewise; the rest of
 *   a segment is left as it was.
 * workspace: dd_range_image_points_workspace_bytes(S, largest H*W), 4-byte aligned.  5 launches per 16 images, no atomics.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer, a non-positive size, a descriptor that leaves its array or overlaps
 * the one before, a workspace that is too small, a misaligned pointer. */
size_t dd_range_image_points_workspace_bytes(int S, long long hw_max);
int dd_range_image_points(const float* range, const int32_t* cp, const float* pose, const double* trig, long long n_total, long long n_pose,
                          long long n_trig, const int32_t* desc, int S, const double* params, int32_t* counts, double* points,
                          int32_t* cp_out, double* rows, void* workspace, size_t workspace_bytes, void* stream);

/* Lens undistortion, cv2.undistort(img, K, dist) with the new camera matrix equal to K (reference prepare_data/waymo.py:10-27):
 * src (n,H,W,3) uint8 -> dst (n,H,W,3) uint8, both 4-byte aligned, frames that share one calibration.  intrinsic [9] float64 on the
 * HOST: f_u, f_v, c_u, c_v, k1, k2, p1, p2, k3.  The source position of every destination pixel in float64 (unfused, in the order
 * csrc/dd_undistort.hip fixes), rounded half to even to 1/32 pixel; bilinear in integers with the weights (32-a)(32-b), a(32-b),
 * (32-a)b, ab, taps outside the image 0, (sum + 512) >> 10; DESIGN 4.23, hipops/undistort.py undistort_host.  One launch.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer, a non-positive size, H*W*3 above 2^31-1, a NaN in the intrinsic or a
 * focal length of 0, a misaligned pointer. */
int dd_undistort(const unsigned char* src, int n, int H, int W, const double* intrinsic, unsigned char* dst, void* stream);

/* Training-mode nn.BatchNorm2d on a channels-last tensor, with the activation that follows it and an optional residual add
 * fused into the normalisation pass: out = act(bn(x) [+ residual]).  Covers torchvision BasicBlock's bn1->relu and
 * bn2(+identity)->relu as used by networks/resnet_encoder.py:42-88, the stem bn1->relu, and LiteMono's BNGELU / DilatedConv.bn1
 * (networks/depth_encoder.py:137-148,197-199).  x, residual, out, g_*: [rows, C] elements of type `dtype` (rows = B*H*W of an NHWC tensor),
 * C a multiple of 4, <= 512.  act: 0 none, 1 ReLU, 2 GELU (erf; not with a residual).  running_mean/var (may both be NULL) are
 * updated in place with `momentum` (unbiased variance, as PyTorch); save_mean/save_invstd [C] feed the backward.
 * Backward: g_x always; g_residual (NULL unless a residual was given and act != 0) = gradient after the activation;
 * `out` (backward): the ReLU mask is read from it when given -- REQUIRED when a residual was added in the forward; NULL for act == 1 without a residual: the mask is recomputed from x (the forward's own fmaf, the same bits), one read pass less.  Batch statistics: sum x and sum x^2 in fp64 from the first addition to the variance, fixed order (no cancellation at mean^2 in fp32).
 * workspace: dd_bn_workspace_bytes(C).  Two launches forward, two backward. */
int dd_bn_act_fwd_t(const void* x, const void* residual, long long rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, float* save_mean, float* save_invstd, int act, void* out, int dtype,
                    void* workspace, size_t workspace_bytes, void* stream);
int dd_bn_act_bwd_t(const void* x, const void* g_out, const void* out, long long rows, int C, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_invstd, int act, void* g_x, void* g_residual, float* g_gamma, float* g_beta,
                    int dtype, void* workspace, size_t workspace_bytes, void* stream);
size_t dd_bn_workspace_bytes(int C);

/* The glue between two 3x3 convolutions of the disparity decoders (reference networks/depth_decoder.py:40-53 Monodepth2,
 * :98-113 Lite-Mono; networks/layers.py:84-121) in one pass, channels-last:
 *     out = ReflectionPad2d(1)( cat( up( act(x) ), skip ) )        out: (B, H+2, W+2, C1+C2)
 * x: (B,h,w,C1) -- with elu != 0 the PRE-activation output of the ConvBlock's convolution, act = ELU(alpha=1), else act = identity;
 * up (mode): 0 nearest x2 (F.interpolate(scale_factor=2, mode="nearest")), 1 bilinear x2 (mode="bilinear", align_corners=False),
 * 2 none (H,W = h,w: ELU + padding only); skip: (B,H,W,C2) or NULL with C2 = 0.  C1, C2 multiples of 4.
 * *_bwd: g_out (B,H+2,W+2,C1+C2) -> g_x (B,h,w,C1) (times ELU'(x) when elu) and g_skip (B,H,W,C2); either may be NULL; gather
 * form, no atomics, overwritten.  dtype: DD_DTYPE_*.  h, w >= 2 and H, W >= 4 (mode 2: h, w >= 4, as dd_reflect_pad1_nhwc_t), anything
 * smaller returns hipErrorInvalidValue and launches nothing.  ELU is expm1(x) for x <= 0 as ATen's, to within 7 x 2^-24 of the value. */
int dd_up_cat_pad_t(const void* x, const void* skip, int B, int h, int w, int C1, int C2, int mode, int elu, void* out, int dtype, void* stream);
int dd_up_cat_pad_bwd_t(const void* g_out, const void* x, int B, int h, int w, int C1, int C2, int mode, int elu, void* g_x, void* g_skip,
                        int dtype, void* stream);

/* LayerNorm over the last (channel) axis of a [rows, C] matrix -- LiteMono's LayerNorm(data_format="channels_last")
 * (networks/depth_encoder.py:101-128, used by LGFI at :241,:252): y = (x - mean) * rstd * gamma + beta, biased variance, eps
 * inside the square root.  x, y, g_out, g_x of type `dtype`; C a multiple of 4, <= 256.  mean, rstd: [rows] fp32, kept for the backward.
 * Backward: g_x [rows, C]; g_gamma_beta [2*C] = (d gamma, d beta), fixed-order column sums.  workspace:
 * dd_layer_norm_workspace_bytes(C).  One launch forward, two backward. */
int dd_layer_norm_fwd_t(const void* x, long long rows, int C, const float* gamma, const float* beta, float eps, void* y, float* mean, float* rstd,
                        int dtype, void* stream);
int dd_layer_norm_bwd_t(const void* x, const void* g_out, const float* gamma, const float* mean, const float* rstd, long long rows, int C,
                        void* g_x, float* g_gamma_beta, void* workspace, size_t workspace_bytes, int dtype, void* stream);
size_t dd_layer_norm_workspace_bytes(int C);

/* Backward of LiteMono's layer-scale residual out = res + y * scale[b,c] (scale = gamma x stochastic-depth factor; reference
 * networks/depth_encoder.py:219-226,266-274): g_y[b,r,c] = g_out[b,r,c] * scale[b,c] and g_scale[b,c] = sum_r g_out * y, one pass.
 * g_out, y, g_y: [B, rows, C] of type `dtype` (rows = H*W of a channels-last image), scale, g_scale: [B, C] fp32; C a multiple of 4, <= 1024.
 * workspace: dd_layer_scale_workspace_bytes(B, C).  The residual's own gradient is g_out itself. */
int dd_layer_scale_bwd_t(const void* g_out, const void* y, const float* scale, int B, int rows, int C, void* g_y, float* g_scale, void* workspace,
                         size_t workspace_bytes, int dtype, void* stream);
size_t dd_layer_scale_workspace_bytes(int B, int C);
/* forward of the layer-scale residual, out = res + y * scale[b, c] (all (B,rows,C) channels-last, scale (B,C) fp32), evaluated in
 * fp32 whatever the storage type: the layer-scale parameters start at 1e-6, below fp16's normal range */
int dd_layer_scale_fwd_t(const void* res, const void* y, const float* scale, int B, int rows, int C, void* out, int dtype, void* stream);

/* The 1x1 reductions of the motion decoders as ONE operator (reference networks/motion_decoder.py:33,66: `refine_motion_redu{level}` =
 * Conv2d(2*ch, out_dim, 1) on cat(a, b)): y[p,co] = bias[co] + sum_c a[p,c] W[co,c] + sum_c b[p,c] W[co,C+c].
 * a, b, g_a, g_b: [P, C] fp32 (channels-last tensors as matrices, P = B*H*W); y, g_out: [P, cout]; weight, g_weight: [cout, 2C] rows (the
 * memory of a (cout, 2C, 1, 1) tensor in either layout); bias, g_bias: [cout] or NULL.  C in {64, 128, 256, 512}, cout in {1, 3}
 * (dd_redu_supported).  Forward one launch, data gradients one launch (either of g_a / g_b may be NULL), weight + bias gradient three
 * launches (per-workgroup partials, two-level fixed-order fold: bit-reproducible); workspace: dd_redu_workspace_bytes(P, C, cout). */
int dd_redu_supported(int C, int cout);
size_t dd_redu_workspace_bytes(long long P, int C, int cout);
int dd_redu_fwd(const float* a, const float* b, const float* weight, const float* bias, long long P, int C, int cout, float* y, void* stream);
int dd_redu_bwd_data(const float* g_out, const float* weight, long long P, int C, int cout, float* g_a, float* g_b, void* stream);
int dd_redu_bwd_weight(const float* a, const float* b, const float* g_out, long long P, int C, int cout, float* g_weight, float* g_bias, void* workspace,
                       size_t workspace_bytes, void* stream);

/* The disparity heads: 3x3, stride-1 convolution to ONE output channel on an input that already carries its reflection padding
 * (reference networks/depth_decoder.py:49-51,95-97 `Conv3x3(num_ch_dec[s], 1)`; the data gradient is dd_conv3x3_cout1_bwd_data).
 * x_padded (B,Hp,Wp,C) channels-last fp32, C = 32 or 64 (dd_conv_head_supported); out / g_out (B,Hp-2,Wp-2).  weight (1,C,3,3) addressed
 * through its element strides; g_weight (3,3,C) dense = the memory order of a channels-last (1,C,3,3) weight; g_bias (1) or NULL.
 * One launch forward; three for the weight + bias gradient (per-workgroup partials, two-level fixed-order fold: bit-reproducible);
 * workspace: dd_conv_head_workspace_bytes(B, Hp, Wp, C). */
int dd_conv_head_supported(int C);
size_t dd_conv_head_workspace_bytes(int B, int Hp, int Wp, int C);
int dd_conv_head_fwd(const float* x_padded, const float* weight, long long s_ci, long long s_kh, long long s_kw, const float* bias, int B, int Hp, int Wp,
                     int C, float* out, void* stream);
int dd_conv_head_bwd_weight(const float* x_padded, const float* g_out, int B, int Hp, int Wp, int C, float* g_weight, float* g_bias, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Convolutions on a handful of channels at full resolution -- the finest level of the motion decoders (reference
 * networks/motion_decoder.py:24-33,57-66: `refine_motion_conv5` = two 3x3 convolutions on 9-12 channels, `refine_motion_redu5` a 1x1
 * reduction to 3 / 1 channels, at 192x640).  stride 1, padding ks/2, dilation 1, groups 1, ks = 1 or 3, fp32.
 * x (B,H,W,cin), y / g_out (B,H,W,cout), g_x (B,H,W,cin): channels-last, dense.  weight: (cout,cin,ks,ks) addressed through its four
 * element strides (any layout).  g_weight: (cout,ks,ks,cin) dense -- the memory order of a channels-last weight tensor; g_bias (cout) or NULL.
 * dd_conv_small_supported: 1 when the (ks, cin, cout) combination is instantiated (forward AND data gradient), else the caller keeps
 * the library's convolution.  workspace: dd_conv_small_workspace_bytes(ks, cin, cout), private to the call's stream.
 * Forward / data gradient: two launches (weight re-ordering, direct convolution); weight gradient: three launches (matrix-pipe
 * partials per workgroup, a two-level fixed-order fold that also yields the bias gradient).  No atomics: bit-reproducible. */
int dd_conv_small_supported(int ks, int cin, int cout);
size_t dd_conv_small_workspace_bytes(int ks, int cin, int cout);
int dd_conv_small_fwd(const float* x, const float* weight, long long s_co, long long s_ci, long long s_kh, long long s_kw, const float* bias, int B, int H,
                      int W, int cin, int cout, int ks, float* y, void* workspace, size_t workspace_bytes, void* stream);
int dd_conv_small_bwd_data(const float* g_out, const float* weight, long long s_co, long long s_ci, long long s_kh, long long s_kw, int B, int H, int W, int cin,
                           int cout, int ks, float* g_x, void* workspace, size_t workspace_bytes, void* stream);
int dd_conv_small_bwd_weight(const float* x, const float* g_out, int B, int H, int W, int cin, int cout, int ks, float* g_weight, float* g_bias,
                             void* workspace, size_t workspace_bytes, void* stream);

/* 3x3 stride-1 convolutions on 16+ channels at fp32 accuracy on the bf16 matrix pipe -- the motion decoders' refinement convolutions
 * (reference networks/motion_decoder.py:24-33,57-66; 64-512 channels per level) and the ResNet encoders' basic blocks (reference
 * networks/resnet_encoder.py via torchvision BasicBlock).  Every fp32 operand is split exactly into three bf16 pieces and each product is
 * formed from six v_mfma_f32_32x32x16_bf16 partial products with fp32 accumulation: the dropped cross terms are at most 2^-23 |x w| (the size of one fp32 rounding), the
 * result has the accuracy of an fp32 FMA chain (csrc/dd_conv_mfma.hip).
 * x (B,Hi,Wi,k_in), y (B,Ho,Wo,n_out): channels-last, dense, fp32; Ho = Hi + 2 pad - 2 (pad 0: pre-padded input, 1: 'same', 2: the data
 * gradient of a pad-0 convolution); x is zero-extended.  k_in % 4 == 0, x 16-byte aligned.
 * dd_conv3x3_mfma_pack: weight (cout,cin,3,3) addressed through its four element strides -> the split weights in matrix-fragment order,
 * pack_fwd (dd_conv3x3_mfma_pack_bytes(cout, cin) bytes) for the forward and / or pack_bwd_data (dd_conv3x3_mfma_pack_bytes(cin, cout)),
 * transposed and mirrored, for the data gradient g_x = dd_conv3x3_mfma(g_out, pack_bwd_data, NULL, ..., k_in = cout, n_out = cin, 2 - pad).
 * dd_conv3x3_mfma_bwd_weight (pad 0 or 1, cin % 4 == cout % 4 == 0): g_weight (cout,3,3,cin) dense -- the memory order of a channels-last
 * weight -- from x and g_out (B,Ho,Wo,cout), the same split arithmetic with the pixels as the contraction; workspace
 * dd_conv3x3_mfma_wgrad_workspace_bytes(B, Ho, Wo, cin, cout), private to the call's stream: one partial per workgroup, folded in a
 * fixed order by a second launch.  No atomics anywhere: every result is bit-reproducible. */
int dd_conv3x3_mfma_supported(int cin, int cout);
size_t dd_conv3x3_mfma_pack_bytes(int n_out, int k_in);
int dd_conv3x3_mfma_pack(const float* weight, long long s_co, long long s_ci, long long s_kh, long long s_kw, int cout, int cin, void* pack_fwd,
                         void* pack_bwd_data, void* stream);
/* The _n forms take the number of partial products per multiply-add: 6 (what the forms without _n compute: fp32 accuracy), 3 = the two
 * leading bf16 pieces of each operand, x1w1 + x1w2 + x2w1 (relative error of a product <= 2^-16: PyTorch's
 * torch.set_float32_matmul_precision("high"), "bf16x3" -- more accurate than the TF32 arithmetic cuDNN runs the reference's fp32
 * convolutions in by default on Ampere-class GPUs), 1 = operands rounded to bf16 ("medium").  Same packs, same layouts, same workspaces. */
int dd_conv3x3_mfma_n(const float* x, const void* pack, const float* bias, int B, int Hi, int Wi, int k_in, int n_out, int pad, int products, float* y,
                      void* stream);
/* The packs of MANY layers in one launch (a network's 3x3 layers at the top of its forward pass instead of one pack launch in front of
 * every convolution).  jobs (device memory): dd_conv3x3_mfma_pack_many_job_words() = 10 64-bit words per layer --
 * { weight pointer, s_co, s_ci, s_kh, s_kw, cout, cin, pack_fwd pointer, pack_bwd_data pointer (0: none), first workgroup of the layer };
 * a layer takes dd_conv3x3_mfma_pack_many_blocks(cout, cin, want_fwd, want_bwd_data) consecutive workgroups; block_job (device memory,
 * n_blocks entries): the layer index of every workgroup.  Every byte written is what dd_conv3x3_mfma_pack writes for that layer
 * (tests/test_conv_mfma_gpu.py::test_packs_of_many_layers_in_one_launch_are_the_single_packs). */
int dd_conv3x3_mfma_pack_many_job_words(void);
int dd_conv3x3_mfma_pack_many_blocks(int cout, int cin, int want_fwd, int want_bwd_data);
int dd_conv3x3_mfma_pack_many(const long long* jobs, const int* block_job, int n_blocks, void* stream);
int dd_conv3x3_mfma(const float* x, const void* pack, const float* bias, int B, int Hi, int Wi, int k_in, int n_out, int pad, float* y, void* stream);
/* The same convolution (pad 1) for SMALL images -- the encoders' and motion decoders' deep levels, 12 x 40 and 6 x 20 pixels with 256 / 512
 * channels -- where 8 x 32-pixel tiles waste half an image and B*H*W / 32 M blocks do not fill the chip: flat 256-pixel tiles of the whole
 * batch, the contraction split across workgroups, partial sums folded in split order (bit-reproducible).  W <= 40, k_in % 4 == 0,
 * n_out % 4 == 0 and 33..64 or > 96 (the two-block pack layout); same packs as dd_conv3x3_mfma (forward: pack_fwd; data gradient: pack_bwd_data on g_out with k_in = cout, n_out = cin).
 * workspace: dd_conv3x3_mfma_flat_workspace_bytes(...) bytes, private to the call's stream. */
int dd_conv3x3_mfma_flat_supported(int B, int H, int W, int k_in, int n_out);
size_t dd_conv3x3_mfma_flat_workspace_bytes(int B, int H, int W, int k_in, int n_out);
int dd_conv3x3_mfma_flat(const float* x, const void* pack, const float* bias, int B, int H, int W, int k_in, int n_out, float* y, void* workspace,
                         size_t workspace_bytes, void* stream);
int dd_conv3x3_mfma_flat_n(const float* x, const void* pack, const float* bias, int B, int H, int W, int k_in, int n_out, int products, float* y,
                           void* workspace, size_t workspace_bytes, void* stream);
size_t dd_conv3x3_mfma_wgrad_workspace_bytes(int B, int Ho, int Wo, int cin, int cout);
int dd_conv3x3_mfma_bwd_weight(const float* x, const float* g_out, int B, int Hi, int Wi, int cin, int cout, int pad, float* g_weight, void* workspace,
                               size_t workspace_bytes, void* stream);
int dd_conv3x3_mfma_bwd_weight_n(const float* x, const float* g_out, int B, int Hi, int Wi, int cin, int cout, int pad, int products, float* g_weight,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The same 3x3 stride-1 convolution for HALF-PRECISION networks (BASELINE.json config 5: "fp16 (CDNA4 MFMA conv)"; the layers of reference
 * networks/resnet_encoder.py:95-135 via torchvision BasicBlock, networks/depth_decoder.py:10-55, networks/motion_decoder.py:24-33,48-66 when
 * the networks run under autocast -- the reference itself has no AMP).  x (B,Hi,Wi,k_in) and y (B,Ho,Wo,n_out) are channels-last, dense, in
 * the half type `dtype` (DD_DTYPE_F16 or DD_DTYPE_BF16); ONE v_mfma_f32_32x32x16_{f16,bf16} per operand pair, fp32 accumulation, fp32 bias
 * (may be NULL), the result rounded to nearest even once (csrc/dd_conv_half.hip).  k_in % 8 == 0, x 16-byte aligned, pad 0..2 as above.
 * dd_conv3x3_half_pack: the fp32 master weight (cout,cin,3,3) addressed through its four element strides -> half-precision fragments,
 * pack_fwd (dd_conv3x3_half_pack_bytes(cout, cin) bytes) and / or pack_bwd_data (dd_conv3x3_half_pack_bytes(cin, cout)), transposed and
 * mirrored, for the data gradient g_x = dd_conv3x3_half(g_out, pack_bwd_data, NULL, ..., k_in = cout, n_out = cin, 2 - pad, ...): the
 * cast autocast would launch per layer happens in the pack.  Bit-reproducible (no atomics, fixed order). */
int dd_conv3x3_half_supported(int cin, int cout);
size_t dd_conv3x3_half_pack_bytes(int n_out, int k_in);
int dd_conv3x3_half_pack(const float* weight, long long s_co, long long s_ci, long long s_kh, long long s_kw, int cout, int cin, int dtype,
                         void* pack_fwd, void* pack_bwd_data, void* stream);
int dd_conv3x3_half(const void* x, const void* pack, const float* bias, int B, int Hi, int Wi, int k_in, int n_out, int pad, int dtype, void* y,
                    void* stream);
/* Its weight gradient (pad 0 or 1, cin % 8 == cout % 8 == 0): g_weight (cout,3,3,cin) dense **fp32** -- the master weights' precision; the
 * products are half x half on the matrix pipe with fp32 accumulation, the pixels as the contraction -- from x and g_out (B,Ho,Wo,cout) in
 * the half type; workspace dd_conv3x3_half_wgrad_workspace_bytes(B, Ho, Wo, cin, cout) bytes, private to the call's stream: one fp32 partial
 * per workgroup, folded in a fixed order by a second launch (no atomics, no zero-fill, no promotion pass; bit-reproducible). */
size_t dd_conv3x3_half_wgrad_workspace_bytes(int B, int Ho, int Wo, int cin, int cout);
int dd_conv3x3_half_bwd_weight(const void* x, const void* g_out, int B, int Hi, int Wi, int cin, int cout, int pad, int dtype, float* g_weight,
                               void* workspace, size_t workspace_bytes, void* stream);

/* LiteMono's point-wise Linears (reference networks/depth_encoder.py:200-203 `pwconv1` / `act` / `pwconv2`, applied at :216-224 and
 * :262-272: nn.Linear(C, 6C) -> nn.GELU() -> nn.Linear(6C, C) on a channels-last (B,H,W,C) tensor, C = 64 / 128 / 224) at fp32 accuracy
 * on the bf16 matrix pipe, with the split arithmetic of dd_conv3x3_mfma (csrc/dd_pw_gemm.hip).
 * dd_pw_gemm: y (M,N) = act(x (M,K)) . W^T + bias, dense row-major fp32; K % 16 == 0, x 16-byte aligned; `pack` holds the split W in
 * matrix-fragment order (dd_pw_gemm_pack_bytes(N, K) bytes); gelu_in != 0 applies the exact (erf) GELU to x while it is split -- the
 * second Linear reads the first one's pre-activation and the activated tensor is never written.  bias may be NULL.
 * dd_mlp_pack: ONE launch packs up to four operands of a block from w1 (hidden,C) and w2 (C,hidden), each addressed through its two
 * element strides: pack_fwd1 (N = hidden, K = C), pack_fwd2 (N = C, K = hidden), and for the data gradients pack_bwd2 = w2 transposed
 * (g_post = g . w2: N = hidden, K = C) and pack_bwd1 = w1 transposed (g_y = g_pre . w1: N = C, K = hidden); NULL skips an operand.
 * dd_mlp_fwd (C = 64, 128 or 224: dd_mlp_fwd_supported): the whole block forward out (M,C) = GELU(x . w1^T + b1) . w2^T + b2 in ONE kernel for
 * passes that keep nothing for a backward (the statistics-only side batch of Trainer.py:215-222's three-frame depth pass, evaluation):
 * the 6C-wide hidden tile stays in accumulator registers between the two GEMMs; operands pack_fwd1 and pack_fwd2_fused
 * (dd_pw_gemm_pack_bytes(C, hidden) bytes: w2 by hidden block, contraction order = the accumulator's register order).
 * dd_mlp_fwd_n: the same with `products` (6 / 3 / 1 as dd_conv3x3_mfma_n) and, at C = 224 -- stage 3's few rows: 128 per workgroup would
 * leave most of the chip idle -- the 42 hidden blocks split over `splits` workgroups per row group (0: dd_mlp_fwd_splits(M, C), chosen so
 * that the grid is one round of the chip; 1..42 forces it): each writes one partial (splits, M, 224) into `workspace`
 * (dd_mlp_fwd_workspace_bytes(M, C, splits) bytes, 16-byte aligned, private to the call's stream; nothing for splits = 1) and a second
 * launch adds them in split order behind b2 (16-byte aligned) -- no atomics, no zero-fill, bit-reproducible for a given split count.
 * C = 64 / 128 take products = 6 and splits <= 1 only (dd_mlp_fwd itself).
 * dd_gelu_pair: the activation's backward in one pass over n elements (n % 4 == 0, 16-byte aligned): post = GELU(pre) (what the second
 * Linear's weight gradient contracts with) and g_inout <- g_inout * GELU'(pre), ATen's arithmetic.  Everything is bit-reproducible. */
size_t dd_pw_gemm_pack_bytes(int N, int K);
int dd_mlp_pack(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden, void* pack_fwd1,
                void* pack_fwd2, void* pack_bwd2, void* pack_bwd1, void* pack_fwd2_fused, void* stream);
int dd_mlp_fwd_supported(int C);
int dd_mlp_fwd(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C, float* y, void* stream);
int dd_mlp_fwd_splits(int M, int C);
size_t dd_mlp_fwd_workspace_bytes(int M, int C, int splits);
int dd_mlp_fwd_n(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C, int products, int splits,
                 float* y, void* workspace, size_t workspace_bytes, void* stream);
int dd_pw_gemm(const float* x, const void* pack, const float* bias, int M, int K, int N, int gelu_in, float* y, void* stream);
int dd_gelu_pair(const float* pre, float* g_inout, float* post, size_t n, void* stream);

/* The TRAINING pass of the block (reference networks/depth_encoder.py:200-203,216-224,262-272: pwconv1 -> GELU -> pwconv2 with a tape, and
 * its data gradient) in dd_mlp_fwd_n's kernels (csrc/dd_pw_gemm.hip: mlp_fwd224_kernel and mlp_fwd_kernel as MLP_TRAIN / MLP_DGRAD).  Written
 * below for the stage-3 block (C = 224, hidden 1344); dd_mlp_train_fwd and dd_mlp_train_bwd also take the narrow widths of stages 1 and 2
 * (C = 64 / 128, hidden 6C, operands from dd_mlp_train_pack_narrow -- dd_mlp_train_pack's arguments and layouts): there the hidden range
 * stays whole (splits 0 or 1 only, anything else is refused; no workspace: dd_mlp_train_bwd_workspace_bytes is 0), y is dd_mlp_fwd's bit for
 * bit at six products, and M * 6C must stay below 2^30.
 * dd_mlp_train_pack: ONE launch writes the four operands a training block needs, each dd_pw_gemm_pack_bytes(hidden, C) bytes, 16-byte
 * aligned: pack_fwd1 and pack_fwd2_fused as dd_mlp_pack writes them, pack_bwd2 = w2 transposed as a first operand (n = hidden, k = C) and
 * pack_bwd1_fused = w1 transposed by hidden block in the accumulator's contraction order (n = C, k = hidden).
 * dd_mlp_train_fwd: y (M,224) = GELU(x . w1^T + b1) . w2^T + b2 exactly as dd_mlp_fwd_n computes it (bit-identical for the same products and
 * splits; workspace dd_mlp_fwd_workspace_bytes), and beside it h = GELU(pre) and d = GELU'(pre) (M,1344 each, dense, 16-byte aligned),
 * stored from the first GEMM's accumulator; rows at or beyond M are never written.
 * dd_mlp_train_bwd: dx (M,224) = ((g . w2) * d) . w1 in one kernel and gpre (M,1344) = (g . w2) * d, the operand of the first Linear's
 * weight gradient (dd_linear_wgrad); the hidden range is split as in the forward, the partials (dd_mlp_train_bwd_workspace_bytes(M, C,
 * splits) bytes, 16-byte aligned, private to the call's stream) folded in split order: no atomics, no zero-fill, bit-reproducible for a
 * given split count.  dd_mlp_train_pack refuses C != 224 and dd_mlp_train_pack_narrow anything but 64 and 128; the two kernels refuse
 * another width, M > 2^19, splits > 42, a short workspace, a pointer that is not 16-byte aligned and products outside {6, 3, 1}. */
int dd_mlp_train_pack(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden, void* pack_fwd1,
                      void* pack_fwd2_fused, void* pack_bwd2, void* pack_bwd1_fused, void* stream);
int dd_mlp_train_fwd(const float* x, const void* pack_fwd1, const void* pack_fwd2_fused, const float* b1, const float* b2, int M, int C, int products,
                     int splits, float* y, float* h, float* d, void* workspace, size_t workspace_bytes, void* stream);
int dd_mlp_train_pack_narrow(const float* w1, long long s1_n, long long s1_k, const float* w2, long long s2_n, long long s2_k, int C, int hidden,
                             void* pack_fwd1, void* pack_fwd2_fused, void* pack_bwd2, void* pack_bwd1_fused, void* stream);
size_t dd_mlp_train_bwd_workspace_bytes(int M, int C, int splits);
int dd_mlp_train_bwd(const float* g, const float* d, const void* pack_bwd2, const void* pack_bwd1_fused, int M, int C, int products, int splits, float* dx,
                     float* gpre, void* workspace, size_t workspace_bytes, void* stream);

/* Weight AND bias gradient of those Linears, and of XCA's qkv / proj (reference networks/depth_encoder.py:200-203, :58-60), in one pass over
 * their operands (csrc/dd_linear_wgrad.hip): g_weight (cout,cin) = g_out^T . x and g_bias (cout) = the column sums of g_out, from the dense
 * row-major fp32 matrices g_out (M,cout) and x (M,cin) (any float alignment: the kernel loads dwords), each read ONCE; the rows are the
 * contraction, with the split arithmetic of dd_conv3x3_mfma_bwd_weight (`products` of the _n form: 6 / 3 / 1 as there).
 * dd_linear_wgrad_supported: M >= 1, cout % 4 == cin % 4 == 0, 4 <= cout, cin <= 8192, and M * max(cout, cin) < 2^30 (the kernel addresses
 * both matrices with 32-bit byte offsets).  workspace: dd_linear_wgrad_workspace_bytes(M, cout, cin) bytes, private to the call's stream -- one partial
 * per workgroup, folded in a fixed order by a second launch that writes every element of both results: no atomics, no zero-fill,
 * bit-reproducible.  g_bias may be NULL. */
int dd_linear_wgrad_supported(int M, int cout, int cin);
size_t dd_linear_wgrad_workspace_bytes(int M, int cout, int cin);
int dd_linear_wgrad(const float* g_out, const float* x, int M, int cout, int cin, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                    void* stream);
int dd_linear_wgrad_n(const float* g_out, const float* x, int M, int cout, int cin, int products, float* g_weight, float* g_bias, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The Adam update of every parameter tensor of a step in ONE launch behind a one-thread-per-tensor prologue (reference Trainer.py:150
 * `optimizer.step()` on torch.optim.Adam, Trainer.py:492-497).  `records` (device memory): one per parameter
 * tensor -- dense fp32 arrays of n elements each, `step` the tensor's step counter as torch keeps it for capturable optimizers (a
 * float on the device; the prologue adds 1 to it, as optimizer.step() does, and evaluates the bias corrections from it).
 * `block_map` (device memory): n_blocks pairs (record index, chunk index), chunk = dd_adam_chunk() elements; the caller lists every
 * chunk of every record once.  `aux`: 8 * n_records bytes of device scratch.  grad_scale / found_inf: NULL, or GradScaler's device
 * scalars (gradients are divided by *grad_scale on the fly -- the gradient arrays are NOT written back --, and nothing is updated,
 * the counters included, when *found_inf != 0).  Update rule and operation order of torch's kernel; bit-reproducible. */
typedef struct DDAdamRecord {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* step;
  long long n;
} DDAdamRecord;
int dd_adam_chunk(void);
int dd_adam_multi(const DDAdamRecord* records, int n_records, const int* block_map, int n_blocks, void* aux, double lr, double beta1, double beta2,
                  double eps, double weight_decay, const float* grad_scale, const float* found_inf, void* stream);

/* Segment visualisation panels on the device (reference eval/visualize.py:24-124 get_vis / combine_vis over Trainer.py:574-605 vis_motion,
 * utils.py:103-164 cart2polar / hsv_to_rgb / score_map_vis; csrc/dd_vis.hip).  A panel is a dense (N, R*H, C*W, 3) uint8 RGB buffer: N frames
 * of R x C tiles of H x W pixels.  `tiles` (host memory): n_tiles <= DD_VIS_MAX_TILES triples { kind, row, col }.
 * dd_vis_frame, once per frame: from that frame's dense fp32 tensors color / ref_color (3,H,W), disp / motion_mask (1,H,W), complete_flow
 * (3,H,W), K / inv_K / cam_T_cam (4,4) it writes the image tiles ((uint8)(x * 255) on x clamped to [0,1]) and the colour-map tiles
 * (matplotlib's Normalize(vmin, vmax) and 256-entry lookup on fp32 data; `lut`: device memory, [2][256] words r | g << 8 | b << 16, the
 * disparity map's table, then the mask's; NaN is black) into frame `frame` of the panel; for every flow tile it stores the pixel's flow
 * magnitude and hue as two fp32 planes of `side` ((max_frames, flow tiles, 2, H, W), the flow tiles in list order) and folds the frame's
 * largest magnitude into maxima[0] (the segment's) and maxima[1 + frame], max_frames + 1 floats the caller zeroes before a segment's first
 * frame: integer atomic maxima on the bit patterns of non-negative floats, so run-to-run identical; nothing returns to the host.  An input
 * that no listed tile reads may be NULL.
 * dd_vis_flow_tiles, once per segment: colours the flow tiles of frames 0 .. n_frames - 1 from `side`, value = clamp(magnitude /
 * (flow_mag_factor * (max + 1e-8)), 0, 1) with the segment's maximum (consistent_flow != 0) or the frame's own, read from `maxima` on
 * the device; rgb = 1 - hsv_to_rgb(hue, 1, value); a list without flow tiles launches nothing.
 * hipErrorInvalidValue: a NULL pointer that a listed tile needs, a non-positive size, a tile outside R x C, more than DD_VIS_MAX_TILES tiles,
 * frame outside 0 .. max_frames - 1. */
#define DD_VIS_MAX_TILES 16
#define DD_VIS_IMG 0
#define DD_VIS_REF_IMG 1
#define DD_VIS_DISP 2
#define DD_VIS_MASK 3
#define DD_VIS_EGO_FLOW 4
#define DD_VIS_IND_FLOW 5
#define DD_VIS_COMP_FLOW 6
#define DD_VIS_SAMP_FLOW 7
int dd_vis_frame(const float* color, const float* ref_color, const float* disp, const float* motion_mask, const float* complete_flow, const float* K,
                 const float* inv_K, const float* cam_T_cam, float min_depth, float max_depth, int H, int W, const int* tiles, int n_tiles, int R, int C,
                 const uint32_t* lut, float disp_vmin, float disp_vmax, float mask_vmin, float mask_vmax, int frame, int max_frames, uint8_t* panel,
                 float* side, float* maxima, void* stream);
int dd_vis_flow_tiles(const float* side, const float* maxima, const int* tiles, int n_tiles, int R, int C, int H, int W, int n_frames,
                      float flow_mag_factor, int consistent_flow, uint8_t* panel, void* stream);

/* Full-resolution depth export (predict.py; csrc/dd_export.hip): the depth metrics' definition of a prediction at a
 * ground-truth pixel -- reference tools.py:42 F.interpolate(disp_scaled, gt size, mode="bilinear", align_corners=False) over
 * tools.py:291-298 disp_to_depth, then 1 / x (tools.py:64) -- at EVERY pixel of the H x W source image, one pass over the output.
 * disp (B,h,w) fp32: the network's sigmoid disparity.  disp_flipped NULL, or (B,h,w): the disparity of the horizontally mirrored
 * image, NOT mirrored back; then l_mask [w] = 1 - clip(20 * (linspace(0,1,w) - 0.05), 0, 1) (host-made table, device memory) and
 * every source tap (y,x) is first fused: l = disp[y,x], r = disp_flipped[y,w-1-x], m = 0.5*(l+r), lm = l_mask[x], rm = l_mask[w-1-x],
 * d = (rm*l + lm*r) + ((1-lm) - rm)*m.  s = lo + span*d as dd_disp_to_depth; u = bilinear(s), d_up = bilinear(d), both fp32 in
 * ATen's order (csrc/dd_bilinear.h) and without fused multiply-add: hipops/export.py export_depth_host is the same arithmetic.
 * Outputs, each NULL or written at every element: depth (B,H,W) fp32 = 1/u; depth16 (B,H,W) = min(rint(depth * depth_scale), 65535)
 * half to even, 0 for NaN and for a product below 0.5; rgb (B,H,W,3) = lut[entry of d_up] by matplotlib's Normalize(vmin, vmax) and
 * 256-entry lookup as dd_vis_frame's disparity tile (lut: 256 words r | g << 8 | b << 16, device memory), black for NaN.
 * dd_export_plane_u8: out (B,H,W) = (uint8)(clamp(bilinear(plane), 0, 1) * 255) of a (B,h,w) fp32 plane -- the motion mask at the
 * source size (reference eval/visualize.py:113-114 shows it at the network's).
 * hipErrorInvalidValue (1), nothing launched: disp / plane / out NULL, no output requested, l_mask without disp_flipped or the
 * reverse, lut without rgb or the reverse, B, h, w, H or W below 1, H*W or h*w above 2^31-1, a non-positive depth bound, a float or
 * table pointer that is not 4-byte aligned, a depth16 pointer that is not 2-byte aligned. */
int dd_export_depth(const float* disp, const float* disp_flipped, const float* l_mask, int B, int h, int w, int H, int W, float min_depth,
                    float max_depth, float depth_scale, const uint32_t* lut, float vmin, float vmax, float* depth, uint16_t* depth16, uint8_t* rgb,
                    void* stream);
int dd_export_plane_u8(const float* plane, int B, int h, int w, int H, int W, uint8_t* out, void* stream);

/* Coloured point clouds (predict.py --save cloud / --scene; csrc/dd_cloud.hip): the depth dd_export_depth writes, at the
 * candidate pixels (Y, X) of the H x W source image with Y % stride == 0 and X % stride == 0, back-projected through a pinhole camera
 * (x right, y down, z forward, integer pixel coordinates as the reference's tools.BackprojectDepth), filtered, optionally moved by a
 * rigid pose and compacted in order into 16-byte records: three little-endian floats x, y, z, then the bytes r, g, b, 255 -- the vertex
 * layout of a binary PLY file.  fp32, unfused; hipops/cloud.py export_cloud_host is the definition in numpy, bit for bit.
 * disp, disp_flipped, l_mask as dd_export_depth.  color (B,3,h,w) in [0,1]: the network-resolution frame; a record's colour is
 * vis_unit_byte of its bilinear sample.  motion_mask NULL or (B,h,w).  pose NULL or (B,3,4) row-major [R | t] per frame.
 * fx, fy, cx, cy: in pixels of the H x W frame; 1/fx and 1/fy are evaluated in double and rounded to fp32 once.
 * Kept: depth > 0 && depth <= max_range; with edge > 0 also (smax - smin) <= edge * smin over the four scaled disparity taps; with a
 * motion mask also bilinear(mask) < motion_thresh.  Every comparison is false for NaN.
 *   point = (((float)X - cx) / fx * depth, ((float)Y - cy) / fy * depth, depth), with a pose p'_k = ((R[k,0] x + R[k,1] y) + R[k,2] z) + t[k].
 * records: room for every candidate, B * ceil(H/stride) * ceil(W/stride) * 16 bytes, 16-byte aligned; the kept candidates of frame 0 in
 *   row-major (Y, X) order, then frame 1, ...; bytes past offsets[B] * 16 are not touched.
 * offsets (B+1) int64: the records of frame b are offsets[b] .. offsets[b+1] - 1.
 * workspace: dd_export_cloud_workspace_bytes(B, H, W, stride), 8-byte aligned; every word the call reads it has written before.
 * Three launches (count, scan, write), integer placement, no atomics: every output byte is the same from run to run.
 * hipErrorInvalidValue (1), nothing launched: disp, color, records, offsets or workspace NULL, l_mask without disp_flipped or the
 * reverse, B, h, w, H, W or stride below 1, H*W or h*w above 2^31-1, more than 2^32 - 1 lanes (B * ceil(H/stride) *
 * ceil(ceil(W/stride) / 256) * 256), fx or fy zero or not finite, a non-positive depth bound, a float pointer that is not 4-byte
 * aligned, records not 16-byte, offsets or workspace not 8-byte aligned, a workspace that is too small (the query returns 0 for sizes
 * that are refused). */
size_t dd_export_cloud_workspace_bytes(int B, int H, int W, int stride);
int dd_export_cloud(const float* disp, const float* disp_flipped, const float* l_mask, const float* color, const float* motion_mask,
                    const float* pose, int B, int h, int w, int H, int W, float fx, float fy, float cx, float cy, float min_depth,
                    float max_depth, float max_range, float edge, float motion_thresh, int stride, void* records, long long* offsets,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Moving objects as labelled instances (predict.py --save objects; csrc/dd_objects.hip): the connected components of the
 * thresholded motion mask and one table row per object.  hipops/objects.py objects_host is the definition in numpy.
 * All maps at the network's resolution: motion_mask (B,h,w), disp, disp_flipped, l_mask as dd_export_depth, complete_flow (B,3,h,w),
 * ts (B), pose (B,3,4) row-major [R | t] of the transform from frame 0 to the neighbouring frame.  fx, fy, cx, cy: in pixels of the
 * h x w image; 1/fx and 1/fy are evaluated in double and rounded to fp32 once.  lo, span: s = lo + span * d, as dd_disp_to_depth makes them.
 * Foreground: motion_mask >= thresh (false for NaN).  A component is a maximal set of foreground pixels of one image connected through
 * 4- or 8-neighbourhoods (connectivity); its anchor is its smallest index y*w + x.  Components of at least min_pixels pixels are the
 * image's objects, numbered 1, 2, ... by increasing anchor; only the first max_objects of them are kept.
 * labels (B,h,w) int32: the number of the pixel's kept object, else 0.
 * counts (B,3) int32: the objects kept, the objects found, 1 where found > max_objects.
 * table (B, max_objects, DD_OBJECTS_ROW 32-bit words), 8-byte aligned; the row of object n of image b is row (b, n-1):
 *   word 0 pixels; 1 x0, 2 y0, 3 x1, 4 y1: the inclusive box; 5 anchor; 6 z_min, 7 z_max as fp32: fminf / fmaxf of z over the
 *   object's pixels with 0 < z < inf, +inf and 0 where it has none; words 8..21 seven doubles: the sums over the object's pixels of
 *   p[3], r[3] and motion_mask, each term the fp32 value below widened, in no fixed order (fp64 atomics).  Rows at and past the
 *   image's kept count are all zero.
 * Per pixel (y, x) of image b, fp32 and unfused: d the (fused) disparity, s = lo + span*d, z = 1/s, p = (xc*z, yc*z, z) with
 *   xc = ((float)x - cx)/fx, yc = ((float)y - cy)/fy;  q_k = ((R[k,0] p0 + R[k,1] p1) + R[k,2] p2) + t[k];  r = complete_flow * ts[b] - (q - p):
 *   the object's own motion between the two frames in frame 0's camera coordinates.  A pixel whose z is NaN, infinite or not
 *   positive still belongs to its object and enters the sums; only that object's row can become NaN.
 * workspace: dd_objects_workspace_bytes(B, h, w, max_objects), 8-byte aligned; every word the call reads it has written before.
 * Five launches (tile, merge, flatten, number, reduce); no workgroup waits for another.
 * dd_export_labels_u16: out (B,H,W) = min(labels[b, min(h-1, (2Y+1)*h / (2H)), min(w-1, (2X+1)*w / (2W))], 65535) in integer
 * arithmetic: the label image at the source size, nearest neighbour.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer other than disp_flipped and l_mask, l_mask without disp_flipped or the
 * reverse, B, h, w (H, W) below 1, B*h*w, H*W or B*max_objects above 2^31-1, connectivity other than 4 and 8, min_pixels below 1,
 * max_objects outside 1..65535, fx or fy zero or not finite, a float, labels or counts pointer that is not 4-byte aligned, table or
 * workspace not 8-byte aligned, out not 2-byte aligned, a workspace that is too small (the query returns 0 for sizes that are refused). */
#define DD_OBJECTS_ROW 22
size_t dd_objects_workspace_bytes(int B, int h, int w, int max_objects);
int dd_objects(const float* motion_mask, const float* disp, const float* disp_flipped, const float* l_mask, const float* complete_flow,
               const float* ts, const float* pose, int B, int h, int w, float fx, float fy, float cx, float cy, float lo, float span, float thresh,
               int connectivity, int min_pixels, int max_objects, int* labels, void* table, int* counts, void* workspace,
               size_t workspace_bytes, void* stream);
int dd_export_labels_u16(const int* labels, int B, int h, int w, int H, int W, uint16_t* out, void* stream);

/* Objects linked across frames (predict.py --save tracks; csrc/dd_tracks.hip): the vote of the network's own
 * correspondences between two label maps.  hipops/tracks.py link_host is the definition in numpy.
 * All maps at the network's resolution: labels_src (B,h,w) int32 the object numbers of frame i (dd_objects' labels), labels_dst (B,h,w)
 * those of its predecessor; disp, disp_flipped, l_mask as dd_objects; complete_flow (B,3,h,w) and ts (B) of the gap to the predecessor.
 * fx, fy, cx, cy: in pixels of the h x w image; 1/fx and 1/fy are evaluated in double and rounded to fp32 once.  lo, span: s = lo + span * d.
 * M = max_objects.  Per pixel (y, x) of image b with a = labels_src in 1..M, fp32 and unfused: d the (fused) disparity, z = 1/(lo + span*d),
 *   p = (xc*z, yc*z, z) with xc = ((float)x - cx)/fx, yc = ((float)y - cy)/fy;  m_k = p_k + complete_flow[b,k,y,x] * ts[b]: the point in the
 *   predecessor's camera, no pose needed;  u = fx*(m0/m2) + cx, v = fy*(m1/m2) + cy;  uf = floorf(u + 0.5f), vf = floorf(v + 0.5f);
 *   inside = m2 > 0 && 0 <= uf <= w-1 && 0 <= vf <= h-1, every comparison false for NaN; the conversion to int happens behind that test.
 *   column = M+1 when not inside, else t = labels_dst[b, (int)vf, (int)uf] where t is in 1..M and 0 otherwise.
 * A source label outside 1..M votes nowhere, a destination label outside 0..M counts as background: whatever the maps hold, no address
 * outside the buffers is formed.
 * votes (B, M, M+2) int32: votes[b, a-1, column] = the number of such pixels; column 0 background, 1..M objects, M+1 outside the image
 *   or behind the camera.  Every word is written by the call.
 * links (B, M, DD_TRACKS_LINK) int32 per row: dst, votes, dst2, votes2, background, outside.  dst: the smallest column of 1..M that holds
 *   the row's largest count over those columns where that count is positive, else 0 with votes 0; dst2: the same over the columns other
 *   than dst; background, outside: columns 0 and M+1.  Rows of numbers no pixel carries are zero.
 * Three launches (memset, vote, select); no workgroup waits for another; integer atomics only: the outputs are the same bytes every run.
 * hipErrorInvalidValue (1), nothing launched: a NULL pointer other than disp_flipped and l_mask, l_mask without disp_flipped or the
 * reverse, B, h, w or max_objects below 1, B*h*w or B*M*(M+2) above 2^31-1, max_objects above DD_TRACKS_MAX_OBJECTS, fx or fy zero or
 * not finite, a pointer that is not 4-byte aligned. */
#define DD_TRACKS_LINK 6
#define DD_TRACKS_MAX_OBJECTS 1024
int dd_tracks_link(const int* labels_src, const int* labels_dst, const float* disp, const float* disp_flipped, const float* l_mask,
                   const float* complete_flow, const float* ts, int B, int h, int w, float fx, float fy, float cx, float cy, float lo, float span,
                   int max_objects, int* votes, int* links, void* stream);

const char* dd_error_string(int code);
int dd_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DYNAMO_HIP_H_ */
