/*
 * lwg.h -- C ABI of liblwg.so, the MI355X (gfx950) native library behind the Imitator.forward()
 * hot path of Liquid Warping GAN (reference: svip-lab/impersonator).
 *
 * This is the drop-in boundary.  The reference's native boundary for this path
 * is the pybind11 module `neural_renderer.cuda.rasterize` (rasterize_cuda.cpp:70-95,194-200) plus the
 * ATen/cuDNN operators PyTorch dispatches for networks/generator.py; liblwg replaces both with plain
 * C entry points: raw device pointers + sizes, no C++ or torch types, never throws, returns 0 or a
 * negative LWG_ERR_* code (text via lwg_last_error()).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - the caller owns every input/output buffer (PyTorch tensors in the Python host code);
 *   - all work is enqueued on the caller's stream (`lwg_stream_t` = hipStream_t), no implicit sync;
 *   - fp32 everywhere, int32 face ids; image tensors are NCHW at the boundary like the reference's,
 *     feature maps handed between entry points are NHWC (== torch.channels_last storage);
 *   - a `lwg_generator` handle owns only what the caller cannot see: re-laid-out weights and scratch.
 *     One handle per device, not to be used from two threads at once.
 */
#ifndef LWG_H_
#define LWG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LWG_API __attribute__((visibility("default")))

typedef void *lwg_stream_t; /* hipStream_t */

enum {
    LWG_OK = 0,
    LWG_ERR_INVALID_ARG = -1, /* NULL pointer, non-positive size, ... (reference: AT_CHECK -> RuntimeError) */
    LWG_ERR_UNSUPPORTED = -2, /* shape outside what the kernels are built for */
    LWG_ERR_WORKSPACE = -3,   /* workspace too small / misaligned */
    LWG_ERR_HIP = -4,         /* a HIP runtime call or kernel launch failed (reference only printf'd these) */
    LWG_ERR_STATE = -5        /* handle not ready (weights missing, batch above max_batch, ...) */
};

LWG_API int lwg_version(void);
/* thread-local text of the last failure in this thread; never NULL */
LWG_API const char *lwg_last_error(void);
/* name may be NULL; returns LWG_ERR_HIP when no device is visible */
LWG_API int lwg_device_info(int *cu_count, size_t *hbm_bytes, char *name_host, size_t name_len);

/* ------------------------------------------------------------------------------------------------
 * Geometry: replaces the python glue in front of the rasteriser.
 * ---------------------------------------------------------------------------------------------- */

/* verts (bs,nv,3), cam (bs,3) = [s,tx,ty], faces_idx (nf,3) -> f2verts (bs,nf,3,3).
 * = orthographic_proj_withz_idrot (utils/nmr.py:10-28) + y flip (nmr.py:271) + nr.look_at with the
 * renderer's eye (0,0,eye_z) (nmr.py:177,273; look_at.py:6-62: identity rotation, z -= eye_z)
 * + nr.vertices_to_faces (vertices_to_faces.py:4-22). */
LWG_API int lwg_project_faces(const float *verts, const float *cam, const int32_t *faces_idx, int bs, int nv,
                              int nf, float eye_z, float *f2verts, lwg_stream_t stream);

/* Rasteriser: replaces rasterize_cuda.forward_face_index_map (rasterize_cuda.cpp:70-95; kernels
 * rasterize_cuda_kernel.cu:40-186) together with the fills of rasterize.py:50-52 and the vertical
 * flips of rasterize.py:334-338.  faces (bs,nf,3,3) -> fim int32 (bs,is,is) [-1 = background],
 * wim (bs,is,is,3) [0 where uncovered], depth (bs,is,is) [far where uncovered] or NULL.
 * Results are bit-identical to the UNcontracted (no fused multiply-add) evaluation of the .cu file's float
 * expressions, lowest face index winning depth ties; nvcc contracts a*b+c by default, which moves the barycentric
 * weights of a CUDA build by the amounts tabulated in profiles/r02_fma_sensitivity.md (coverage and face indices: 0).
 * Stateless between calls (the workspace is scratch for the duration of one call): no global atomics, no depth buffer
 * in memory.  workspace: lwg_rasterize_workspace_bytes, 256-byte aligned. */
LWG_API size_t lwg_rasterize_workspace_bytes(int bs, int nf, int image_size);
LWG_API int lwg_rasterize_fim_wim(const float *faces, int bs, int nf, int image_size, float near_z, float far_z,
                                  int32_t *fim, float *wim, float *depth, void *workspace, size_t workspace_bytes,
                                  lwg_stream_t stream);

/* SMPLRenderer.encode_fim (utils/nmr.py:328-341): out = map_fn[fim] with fim == -1 -> last row.
 * map_fn (nrows,nc); fim (bs,npix); out (bs,nc,npix) when transpose != 0 else (bs,npix,nc). */
LWG_API int lwg_encode_fim(const int32_t *fim, const float *map_fn, int bs, int npix, int nrows, int nc,
                           int transpose, float *out, lwg_stream_t stream);

/* SMPLRenderer.cal_bc_transform (utils/nmr.py:617-659): T = sum_k wim[k] * src_f2pts[fim][k] on
 * covered pixels, (-2,-2) elsewhere.  src_f2pts (src_bs,nf,3,2) with src_bs == 1 (shared) or bs. */
LWG_API int lwg_cal_bc_transform(const float *src_f2pts, int src_bs, const int32_t *fim, const float *wim, int bs,
                                 int nf, int image_size, float *T, lwg_stream_t stream);

/* F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros') as called at models/imitator.py:259 and
 * networks/generator.py:313.  x (xn,C,H,W) NCHW with xn == 1 (shared) or n; grid (n,Ho,Wo,2);
 * out (n,C,Ho,Wo).  align_corners: 0 = torch>=1.3 default (parity target), 1 = torch 1.2 behaviour (H1). */
LWG_API int lwg_grid_sample(const float *x, int xn, int C, int H, int W, const float *grid, int n, int Ho, int Wo,
                            int align_corners, float *out, lwg_stream_t stream);

/* ImpersonatorGenerator.resize_trans (networks/generator.py:303-310): bilinear, align_corners=True,
 * of the flow field T (bs,H,W,2) -> (bs,h,w,2). */
LWG_API int lwg_resize_flow(const float *T, int bs, int H, int W, int h, int w, float *out, lwg_stream_t stream);

/* GlobalLocalDiscriminator.crop_body (networks/discriminator.py:80-96): out[i] = F.interpolate(x[i, :, min_y:max_y, min_x:max_x],
 * size=(S,S), mode='bilinear', align_corners=True).  x, out (n,C,S,S) NCHW (the layout lwg_discriminator_forward takes);
 * boxes (n,4) int64 IN DEVICE MEMORY, (min_x, max_x, min_y, max_y) with exclusive ends -- what cal_body_bbox / cal_head_bbox
 * (models/impersonator_trainer_aug.py:86-166) return.  The kernel reads the boxes itself: no host read, no synchronisation,
 * no allocation, so a captured graph replays with whatever boxes the tensor then holds.  Every coordinate is clamped to [0,S]
 * before use; a sample whose clamped box is empty (max <= min on either axis) gets zeros.  PyTorch's align-corners arithmetic
 * per axis: scale = (in-1)/(S-1) (0 for in == 1), src = scale*dst, i0 = floor(src), lambda = src - i0, i1 = i0 + (i0 < in-1).
 * S <= 1024, n*C <= 65535. */
LWG_API int lwg_crop_resize(const float *x, int n, int C, int S, const int64_t *boxes, float *out, lwg_stream_t stream);
/* Its exact adjoint (what autograd does behind crop_body under loss.backward(), impersonator_trainer_aug.py:365): dy (n,C,S,S)
 * -> dx (n,C,S,S), WRITTEN (not accumulated), 0.0 outside each box.  A column gather followed by a row gather in a fixed order,
 * no atomics: bit-reproducible from run to run. */
LWG_API int lwg_crop_resize_backward(const float *dy, int n, int C, int S, const int64_t *boxes, float *dx,
                                     lwg_stream_t stream);

/* One launch sequence for models/imitator.py:250-260 given posed vertices:
 * project -> rasterise -> cond = map_fn[fim] -> T -> tsf_img = grid_sample(src_img, T)
 * -> tsf_inputs = cat(tsf_img, cond).  Shared source: src_p2verts (nf,3,2), src_img (3,is,is).
 * Outputs (any of cond/tsf_img/tsf_inputs_nhwc8 may be NULL): f2verts (bs,nf,3,3), fim, wim,
 * cond (bs,nc,is,is), T (bs,is,is,2), tsf_img (bs,3,is,is), tsf_inputs_nhwc8 (bs,is,is,8) =
 * [tsf_img(3), cond(nc=3), 0, 0] per pixel -- the layout lwg_generator_* consumes directly. */
LWG_API size_t lwg_transfer_workspace_bytes(int bs, int nf, int image_size);
LWG_API int lwg_transfer_frame(const float *verts, const float *cam, const int32_t *faces_idx, int bs, int nv, int nf,
                               int image_size, float eye_z, float near_z, float far_z, const float *map_fn, int nc,
                               const float *src_p2verts, const float *src_img, int align_corners, float *f2verts,
                               int32_t *fim, float *wim, float *cond, float *T, float *tsf_img,
                               float *tsf_inputs_nhwc8, void *workspace, size_t workspace_bytes,
                               lwg_stream_t stream);

/* SMPL.forward (networks/batch_smpl.py:285-375) for a batch of frames: theta (bs, 3+72+num_betas) =
 * [cam, pose, shape] -> verts (bs,nv,3), joints (bs,num_out_joints,3) [optional], Rs (bs,24,3,3) [optional].
 * Model tensors in the reference's own layouts: v_template (nv,3), shapedirs (num_betas, nv*3),
 * posedirs (207, nv*3), weights (nv,24), joint_regressor (nv,num_out_joints), parents (24).
 * J_template (24,3) and J_shapedirs (num_betas, 72) are the joint regressor applied to v_template / shapedirs
 * (the regression J_regressor^T v_shaped of batch_smpl.py:318-321 is linear in the shape; precomputed once). */
/* The tensor glue around SMPL.forward on the per-frame path, as two launches.
 * smpl_swap: Imitator.swap_smpl (models/imitator.py:216-234) + the slicing of HumanModelRecovery.get_details
 *   (networks/hmr.py:302-330): tgt_smpl (bs, 75+num_betas) -> theta (bs, 75+num_betas) = [cam, tgt pose, src shape] and its
 *   contiguous parts cam (bs,3), pose (bs,72), shape (bs,num_betas).  strategy 1 'smooth': cam = [src_s, src_t + (tgt_t -
 *   first_t)]; 2 'source': src_cam; 3 'copy': the target's own camera; 0: theta = tgt_smpl unchanged (get_details only).
 *   src_cam (3), src_shape (num_betas), first_cam (3): device pointers, NULL where the strategy does not read them.
 * smpl_project_joints: batch_orth_proj_idrot (networks/batch_smpl.py:221-234): j2d (bs,J,2) = cam_s * (j3d_xy + cam_t). */
LWG_API int lwg_smpl_swap(const float *tgt_smpl, int bs, int num_betas, int strategy, const float *src_cam,
                          const float *src_shape, const float *first_cam, float *theta, float *cam, float *pose, float *shape,
                          lwg_stream_t stream);
LWG_API int lwg_smpl_project_joints(const float *j3d, const float *cam, int bs, int num_joints, float *j2d, lwg_stream_t stream);
/* Viewer.rotate_trans (models/viewer.py:240-247), `torch.bmm(X, R) + t` of the novel-view path: out (n,3) = x (n,3) @ R + t.
 * R9 (row-major 3x3) and t3 are HOST pointers (twelve floats, passed to the kernel by value); x / out device pointers. */
LWG_API int lwg_rotate_translate(const float *x, long n, const float *R9, const float *t3, float *out, lwg_stream_t stream);
/* The same mesh under n rigid transforms at once (a turntable of novel views): x (nv,3) -> out (n,nv,3), out[k] = x @ R_k + t_k.
 * Rt (n,12) is a DEVICE array, row k = [R_k row-major (9), t_k (3)]: the kernel reads it, so a captured graph replays with
 * whatever the table holds then.  out[k] is bit-identical to lwg_rotate_translate with the same twelve numbers.  n <= 65535. */
LWG_API int lwg_rigid_views(const float *x, long nv, const float *Rt, int n, float *out, lwg_stream_t stream);
LWG_API size_t lwg_smpl_workspace_bytes(int bs);
LWG_API int lwg_smpl_forward(const float *theta, int bs, int num_betas, int nv, int num_out_joints,
                             const float *v_template, const float *shapedirs, const float *posedirs,
                             const float *J_template, const float *J_shapedirs, const int32_t *parents,
                             const float *weights, const float *joint_regressor, float *verts, float *joints,
                             float *Rs, void *workspace, size_t workspace_bytes, lwg_stream_t stream);
/* The same function with every intermediate in fp64 and ONE rounding to fp32 at the end ("compensated" mode of
 * networks/batch_smpl.py:285-375): the fp32 model tensors are read as they are, J_template / J_shapedirs are the fp64
 * products of the fp32 regressor with the fp32 template / shape directions.  The result is the correctly rounded value of
 * the function the reference's code defines; any fp32 evaluation of it (the reference's own included) differs from that by
 * its ~1e-6 of summation noise, which the rasteriser downstream amplifies. */
LWG_API int lwg_smpl_forward_f64(const float *theta, int bs, int num_betas, int nv, int num_out_joints,
                                 const float *v_template, const float *shapedirs, const float *posedirs,
                                 const double *J_template, const double *J_shapedirs, const int32_t *parents,
                                 const float *weights, const float *joint_regressor, float *verts, float *joints,
                                 float *Rs, void *workspace, size_t workspace_bytes, lwg_stream_t stream);

/* The mask bookkeeping of appearance transfer, models/swapper.py:198-253 (Swapper.swap / calculate_trans), batch 1 as the reference
 * runs it, NCHW fp32.  With these a swap launches no framework kernel and never reads the device back (the reference's
 * `T11[~src_left_mask[0]] = -2` does), so the whole call can be captured in a HIP graph.
 *   lwg_swap_masks  : part (nparts,H,W) = source part map (encode_fim with the 'par' table); bit c of selected_bits / left_bits = part c
 *                     belongs to the swapped / the kept set.  -> part_mask, left_mask (H,W) in {0,1} = (channel sum != 0), and
 *                     T11 (H,W,2) = grid where left_mask else -2 (grid: the identity sampling grid, utils/nmr.py:490-504).
 *   lwg_mask_faces  : out = f2pts with the faces flagged in `drop` (one byte per face) set to -2 (tsf_f2p[0, left_faces] = -2).
 *   lwg_swap_compose: out (3+nc,H,W) = cat([tsf21 * part_mask + tsf11 * left_mask, cond]).
 *   lwg_clamp       : x = min(max(x, lo), hi) in place (T21.clamp_(-2, 2)). */
LWG_API int lwg_swap_masks(const float *part, int nparts, int H, int W, unsigned selected_bits, unsigned left_bits, const float *grid,
                           float *part_mask, float *left_mask, float *T11, lwg_stream_t stream);
LWG_API int lwg_mask_faces(const float *f2pts, const unsigned char *drop, int nf, int per_face, float *out, lwg_stream_t stream);
LWG_API int lwg_swap_compose(const float *tsf21, const float *tsf11, const float *part_mask, const float *left_mask, const float *cond,
                             int nc, int H, int W, float *out, lwg_stream_t stream);
LWG_API int lwg_clamp(float *x, size_t n, float lo, float hi, lwg_stream_t stream);
/* *out (device) = max |a[i] - b[i]| over n floats; a NaN difference reports +inf.  The comparison behind the generator's
 * `precision="auto"` (impersonator_amd/networks/generator.py): the reference computes networks/generator.py:80-133 in fp32
 * throughout, the library's bf16x3 arithmetic is narrower -- one probe pass in both arithmetics per weight set decides which one
 * serves it, and this is its `(a - b).abs().max()` without a framework kernel. */
LWG_API int lwg_max_abs_diff(const float *a, const float *b, size_t n, float *out, lwg_stream_t stream);
/* The per-frame geometry of Animator (impersonator_amd/models/animator.py: appearance transfer driven by a motion sequence) as ONE
 * launch, one lane per pixel.  The reference's models/animator.py cannot run against its own utils/nmr.py, so the semantics are
 * those of Swapper.swap (models/swapper.py:198-253) with the source's raster maps replaced by the driven pose's:
 *   cond = map_fn[fim];  T_x = clamp(cal_bc_transform(x_f2p, fim, wim), -2, 2) for x in {src, ref};
 *   tsf_img = grid_sample(ref_img, T_ref) * part_mask + grid_sample(src_img, T_src) * left_mask;  tsf_inputs = cat(tsf_img, cond).
 * Inputs: fim (bs,is,is) int32 and wim (bs,is,is,3) as lwg_rasterize_fim_wim writes them; map_fn (nf+1,nc); side (nf+1) bytes, the
 * background row included: bit 0 = the row's selected part channels sum to non-zero (part_mask), bit 1 = its kept channels do
 * (left_mask) -- part = part_fn[fim], so the per-pixel channel sums of the reference are a property of the row; src_f2p / ref_f2p
 * (nf,3,2), shared by the batch, already masked with lwg_mask_faces (ref: the kept parts' faces at -2, src: every other face);
 * src_img / ref_img (3,is,is).  Outputs, any of which may be NULL except the two flows: T_src, T_ref (bs,is,is,2),
 * cond (bs,nc,is,is), tsf_img (bs,3,is,is), tsf_inputs (bs,3+nc,is,is) NCHW, tsf_inputs_nhwc8 (bs,is,is,8) = [tsf_img(3), cond(3),
 * 0, 0] per pixel (nc == 3 only; the layout lwg_generator_* consumes directly).
 * Every output is bit-identical to the chain lwg_encode_fim, lwg_cal_bc_transform, lwg_clamp, lwg_grid_sample, lwg_swap_compose on
 * the same inputs (same float expressions in the same order, no contraction). */
LWG_API int lwg_animate_inputs(const int32_t *fim, const float *wim, int bs, int nf, int image_size, const float *map_fn, int nc,
                               const unsigned char *side, const float *src_f2p, const float *ref_f2p, const float *src_img,
                               const float *ref_img, int align_corners, float *T_src, float *T_ref, float *cond, float *tsf_img,
                               float *tsf_inputs, float *tsf_inputs_nhwc8, lwg_stream_t stream);
/* A batch of images as one uint8 picture: torchvision.utils.make_grid followed by save_image's conversion, which is how the
 * reference's run_view.py:76-85 writes its novel views.  x (n,3,H,W) fp32 NCHW -> out (grid_h,grid_w,3) uint8 HWC.
 *   layout: xmaps = min(nrow, n), ymaps = ceil(n / xmaps); grid_h = (H+padding)*ymaps + padding, grid_w = (W+padding)*xmaps +
 *     padding; image k at row (k / xmaps)*(H+padding) + padding, column (k % xmaps)*(W+padding) + padding; pad_value everywhere
 *     else, the cells of an incomplete last row included.  n == 1: the grid is the image itself, H x W, no padding.
 *   value : v = normalize ? (p + 1) / 2 : p, then uint8(clamp(v * 255 + 0.5, 0, 255)) with truncation; every step a separately
 *     rounded fp32 operation (no fused multiply-add).  pad_value takes the same conversion without the normalize step.
 * lwg_image_grid_shape needs no device.  n, H, W, nrow <= 0 or padding < 0: LWG_ERR_INVALID_ARG. */
LWG_API int lwg_image_grid_shape(int n, int H, int W, int nrow, int padding, int *grid_h, int *grid_w);
LWG_API int lwg_image_grid_u8(const float *x, int n, int H, int W, int nrow, int padding, float pad_value, int normalize,
                              unsigned char *out, lwg_stream_t stream);
/* Baseline sequential JFIF (JPEG) encoder: x (N,3,H,W) fp32 NCHW in [-1,1] -- what Imitator.forward returns -- -> N finished
 * .jpg streams, byte-identical to libjpeg's baseline encoder with its default Huffman tables on the uint8 image
 * trunc(((x + 1) / 2) * 255) (utils/cv_utils.py: save_cv2_img, normalize=True; clamped, NaN -> 0).  The algorithm is stated in
 * csrc/jpeg.hip.  Frame n's stream is out[n * row_stride ... + lengths[n]); bytes behind it are unspecified.
 *   subsampling: 420 (4:2:0) or 444 (4:4:4); quality 1..100 (libjpeg's scaling of the Annex K tables).
 *   lwg_jpeg_stream_bytes: the most a stream can take, 623 + 2 * ceil(nblocks * 1658 / 8) + 2 (a block emits at most 1658 bits,
 *     every byte may be stuffed) -- the least row_stride; lwg_jpeg_workspace_bytes: scratch of one call.  Both need no device and
 *     return 0 for sizes lwg_jpeg_encode refuses.
 *   Stream-ordered: no host synchronisation, no host-to-device copy (capturable in a graph); deterministic byte for byte.
 * NULL pointers, N / H / W <= 0, quality outside 1..100, an unknown subsampling, x or lengths not 4-byte or the workspace not
 * 16-byte aligned: LWG_ERR_INVALID_ARG; H or W not a multiple of 16: LWG_ERR_UNSUPPORTED; a short workspace or row_stride:
 * LWG_ERR_WORKSPACE -- all before the first HIP call. */
LWG_API size_t lwg_jpeg_stream_bytes(int H, int W, int subsampling);
LWG_API size_t lwg_jpeg_workspace_bytes(int N, int H, int W, int subsampling);
LWG_API int lwg_jpeg_encode(const float *x, int N, int H, int W, int quality, int subsampling, uint8_t *out, size_t row_stride,
                            int32_t *lengths, void *workspace, size_t workspace_bytes, lwg_stream_t stream);
/* ---- Paired evaluation of generated frames (csrc/eval.hip): the reference's SSIMMetric, PSNRMetric and ScaleShapePoseError
 * (thirdparty/his_evaluators/.../metrics/metrics.py) without taking a float frame to the host.
 * eval_pair_stats: pred, ref (N,3,H,W) fp32 NCHW -> stats (N,4) FP64 [mssim, mse, ref_min, ref_max] per frame.
 *   mode 0: values as they are ([-1,1], what the generator emits);
 *   mode 1: inputs in [0,1], mapped as the reference's `preprocess` does: fl32(fl32(2*x) - 1);
 *   mode 2: [-1,1] through the 8 bits between writer and loader: u = clamp(trunc(fl32(fl32(fl32(x+1)/2)*255)), 0, 255)
 *           (utils/cv_utils.py: save_cv2_img, normalize=True), v = fl32(fl32(fl32(u)/255)*2) - 1.  JPEG loss is not modelled.
 *   mssim: scikit-image 0.16.2 structural_similarity(multichannel=True) on float32 images: 7x7 uniform window, data_range 2,
 *     K1 0.01, K2 0.03 (C1 4e-4, C2 3.6e-3), cov_norm 49/48, S averaged over the (H-6)x(W-6) window positions inside the image per
 *     channel, then over the three channels.  mse: mean of (pred-ref)^2 over all 3*H*W values.  ref_min / ref_max: over the
 *     mapped ref (PSNR's data_range is 1 when ref_min >= 0, else 2; psnr = 10 log10(data_range^2 / mse), left to the caller).
 *   Pixels are mapped in fp32; window sums, S and every mean are fp64.  Per-tile partials go to the workspace in a fixed layout
 *   and are added in a fixed order: no atomics, bit-reproducible, and a frame's numbers do not depend on N or on its position
 *   in the batch.  Stream-ordered, no host synchronisation.  lwg_eval_workspace_bytes needs no device (0 for sizes <= 0).
 *   NULL, N / H / W <= 0, an unknown mode, stats or workspace not 8-byte aligned: LWG_ERR_INVALID_ARG; H < 7 or W < 7 (scikit-image
 *   raises there) or N > 21845: LWG_ERR_UNSUPPORTED; a short workspace: LWG_ERR_WORKSPACE -- all before the first HIP call.
 * resize_bilinear: F.interpolate(x, (Ho,Wo), mode='bilinear', align_corners=False), no antialiasing, x (N,C,H,W) -> y (N,C,Ho,Wo).
 *   ATen's arithmetic per axis, float32: scale = (float)in / (float)out, src = max(fmaf(scale, dst+0.5f, -0.5f), 0) (the one fused
 *   multiply-add: torch's binaries contract this expression; the lerps below round per step),
 *   i0 = (int)src, i1 = min(i0+1, in-1), l = src - i0; value = (1-ly)*((1-lx)*a00 + lx*a01) + ly*((1-lx)*a10 + lx*a11).
 *   (lwg_resize_flow above is the align_corners=True resize of the flow field.)
 * eval_sspe_terms: pred_theta, ref_theta (N,85) fp32 -> terms (N,3) FP64 per frame: |d[0]|, sum |d[75:85]|, sum |d[0:75]| of
 *   d = pred - ref taken in fp64 -- ssp_abs_err_score_func's scale, shape and "pose" terms, the last covering the camera again. */
LWG_API size_t lwg_eval_workspace_bytes(int N, int H, int W);
LWG_API int lwg_eval_pair_stats(const float *pred, const float *ref, int N, int H, int W, int mode, double *stats, void *workspace,
                                size_t workspace_bytes, lwg_stream_t stream);
LWG_API int lwg_resize_bilinear(const float *x, int N, int C, int H, int W, int Ho, int Wo, float *y, lwg_stream_t stream);
LWG_API int lwg_eval_sspe_terms(const float *pred_theta, const float *ref_theta, int N, double *terms, lwg_stream_t stream);
/* ---- Once-per-source glue of Imitator.personalize (models/imitator.py:82-155), so that `personalize` launches no
 * framework kernel.
 * morph: utils/util.py:73-89 -- erode (mode 0: pad with 1, count == ks*ks) / dilate (mode 1: pad with 0, count >= 1) of a
 *   mask with a ks x ks box (ks odd, <= 31); mask (n,1,H,W) fp32 whose images sit batch_stride floats apart (a channel slice of
 *   an NCHW tensor qualifies), out (n,1,H,W) dense.  Exact for {0,1} masks (integer counts).  complement != 0 writes
 *   1 - result (body_mask = 1 - bg_mask, ft_mask = 1 - erode: imitator.py:117,134).
 * mask_compose: torch.cat([img * m, tail], dim=1) with m = mask or 1 - mask (invert): img (n,3,H,W), mask (n,1,H,W), tail
 *   (n,tail_channels,H,W) -> out (n,3+tail_channels,H,W) (imitator.py:127-128,135).
 * source_p2verts: hazard H9 (imitator.py:105-107): negates y of f2verts (bs,nf,3,3) IN PLACE (the reference does it through
 *   the p2verts view) and writes the contiguous p2verts (bs,nf,3,2) = f2verts[..., 0:2].
 * vis_f2pts: SMPLRenderer.get_vis_f2pts (utils/nmr.py:506-546, --only_vis, hazard H10): out = f2pts (bs,nf,per_face floats per
 *   face) where the face id is among fim.unique()[1:] -- the sorted unique values minus the SMALLEST one present, whatever it
 *   is -- and -2 elsewhere. */
LWG_API int lwg_morph(const float *mask, int n, int H, int W, long batch_stride, int ks, int mode, int complement, float *out,
                      lwg_stream_t stream);
LWG_API int lwg_mask_compose(const float *img, const float *mask, int invert, const float *tail, int tail_channels, int n,
                             int H, int W, float *out, lwg_stream_t stream);
LWG_API int lwg_source_p2verts(float *f2verts, int bs, int nf, float *p2verts, lwg_stream_t stream);
LWG_API size_t lwg_vis_f2pts_workspace_bytes(int bs, int nf);
LWG_API int lwg_vis_f2pts(const float *f2pts, int bs, int nf, int per_face, const int32_t *fim, int H, int W, float *out,
                          void *workspace, size_t workspace_bytes, lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Textured rendering (render.hip): the shading half of SMPLRenderer (utils/nmr.py:192-244,295-310,354-388) on top of
 * lwg_project_faces + lwg_rasterize_fim_wim.  Forward only.
 * face_light: neural_renderer/lighting.py:33-53 per face on the RAW vertices: verts (bs,nv,3), faces_idx (nf,3) ->
 *   light (bs,nf,3) = int_amb * color_amb + int_dir * color_dir * relu(dot(n, direction)), n = cross(v0-v1, v2-v1) /
 *   max(|cross|, 1e-5); direction is used as given; a term whose intensity is 0 is skipped.  The three colour / direction
 *   triples are HOST pointers.
 * shade_resolve: rasterize_cuda_kernel.cu:207-259 + rasterize.py:190-197 + :343.  f2verts (bs,nf,3,3); fim / wim / depth as
 *   lwg_rasterize_fim_wim writes them at S = image_size * (anti_aliasing ? 2 : 1); textures (tex_bs,nf,ts,ts,ts,3) and
 *   background (bg_bs,3) with a batch of 1 (shared) or bs; light (bs,nf,3) -> rgb (bs,3,image_size,image_size).  Covered
 *   sub-pixels (0 <= fim < nf) take the eight-corner blend at tif[k] = w[k] * (ts-1) * (depth / z_k) clamped to
 *   [0, (ts-1) - eps], times the face's light; the others the background; anti_aliasing averages the 2x2 sub-pixels.
 *   tex_size >= 2.
 * silhouette_resolve: fim at S -> alpha (bs,image_size,image_size): fim >= 0, averaged over 2x2 with anti_aliasing.
 * face_sampler: SMPLRenderer.dynamic_sampler (nmr.py:382-388): p = s * (X_xy + t) (no y flip), then per face and per column
 *   t of coords (2,tex_points): (v0-v2) * c0 + (v1-v2) * c1 + v2 clamped to [-1,1] -> sampler (bs,nf,tex_points,2).
 * extract_tex: SMPLRenderer.extract_tex (nmr.py:364-380): uv_img (img_bs,3,H,W), img_bs 1 or bs; sampler (bs,nf,ts*ts,2)
 *   -> tex (bs,nf,ts,ts,ts,3), the bilinear sample (bit-identical to lwg_grid_sample on the same grid) repeated along the
 *   third texture axis. */
LWG_API int lwg_face_light(const float *verts, const int32_t *faces_idx, int bs, int nv, int nf, float intensity_ambient,
                           float intensity_directional, const float *color_ambient_host, const float *color_directional_host,
                           const float *direction_host, float *light, lwg_stream_t stream);
LWG_API int lwg_shade_resolve(const float *f2verts, const int32_t *fim, const float *wim, const float *depth,
                              const float *textures, int tex_bs, const float *light, const float *background, int bg_bs, int bs,
                              int nf, int image_size, int anti_aliasing, int tex_size, float eps, float *rgb,
                              lwg_stream_t stream);
LWG_API int lwg_silhouette_resolve(const int32_t *fim, int bs, int image_size, int anti_aliasing, float *alpha,
                                   lwg_stream_t stream);
LWG_API int lwg_face_sampler(const float *cam, const float *verts, const int32_t *faces_idx, const float *coords, int bs, int nv,
                             int nf, int tex_points, float *sampler, lwg_stream_t stream);
LWG_API int lwg_extract_tex(const float *uv_img, int img_bs, int H, int W, const float *sampler, int bs, int nf, int tex_size,
                            int align_corners, float *tex, lwg_stream_t stream);

/* NCHW (n,C,H,W) -> NHWC with the channel count padded to cpad (zeros), and back (first C channels). */
LWG_API int lwg_pack_nhwc(const float *x_nchw, int n, int C, int H, int W, int cpad, float *out_nhwc,
                          lwg_stream_t stream);
LWG_API int lwg_unpack_nchw(const float *x_nhwc, int n, int C, int H, int W, int cpad, float *out_nchw,
                            lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Generator: replaces what PyTorch dispatches for ImpersonatorGenerator (networks/generator.py:187-320):
 * conv / conv-transpose / InstanceNorm / ReLU / grid_sample / interpolate / cat / tanh / sigmoid.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lwg_generator lwg_generator;

/* ImpersonatorGenerator(bg_dim, src_dim, tsf_dim, conv_dim=64, repeat_num=6), n_down = 3
 * (generator.py:189-202).  Allocates weights + scratch for batches up to max_batch.  src_dim / tsf_dim = 3 + the condition
 * map's channels (models/models.py:85-94, utils/mesh.py:446-473): 1..32, i.e. every map_name of the reference ('uv_seg' 6,
 * 'par' 14, 'binary' 18).  Inputs of at most 8 channels take the NHWC8 path (layout 1 of lwg_generator_inference) and, under
 * precision 1, the LDS-resident bf16x3 stem; wider ones are NCHW only and their 7x7 stem runs on the exact-fp32 kernel. */
LWG_API int lwg_generator_create(lwg_generator **out, int src_dim, int tsf_dim, int conv_dim, int repeat_num,
                                 int image_size, int max_batch);
LWG_API void lwg_generator_destroy(lwg_generator *g);

/* Arithmetic of the convolutions.  0: exact fp32 on v_mfma_f32_32x32x2_f32 (bit-for-bit an fmaf chain).
 * 1 (default): every fp32 operand split into two bf16 terms, hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation -- 16 mantissa bits per operand, ~2^-16 relative per product, measured 8e-5 L-inf on the final
 * image against the fp32 reference (budget 1e-3), at ~2.2x the speed.  The 7x7 stem and heads are fp32 in both modes. */
LWG_API int lwg_generator_set_precision(lwg_generator *g, int mode);

/* Batched forms for ImpersonatorGenerator.infer_front / forward (generator.py:204-243: one source per sample, both
 * streams decoded).  encode_src_n: src_inputs (bs,src_dim,is,is) -> the same feature list with batch bs.
 * decode_src: src_model.regress(src_model.decode(...)) on those features -> color (bs,3,is,is), mask (bs,1,is,is).
 * inference_n: lwg_generator_inference with feats_bs in {1, bs} sources. */
LWG_API int lwg_generator_encode_src_n(lwg_generator *g, const float *src_inputs_nchw, int bs, float *const *feats_nhwc,
                                       lwg_stream_t stream);
LWG_API int lwg_generator_decode_src(lwg_generator *g, const float *const *feats_nhwc, int bs, float *color, float *mask,
                                     lwg_stream_t stream);
LWG_API int lwg_generator_inference_n(lwg_generator *g, const float *tsf_inputs, int layout, const float *T, int bs,
                                      const float *const *feats_nhwc, int feats_bs, int align_corners, float *color,
                                      float *mask, const float *bg, int bg_bs, float *pred, lwg_stream_t stream);

/* BGNet = ImpersonatorGenerator.bg_model (ResNetGenerator, networks/generator.py:23-65), used by Imitator.personalize
 * when --bg_model ORIGINAL (models/imitator.py:30-34, 127-132).  enable_bg allocates its weights (call before feeding
 * "bg_model.*" keys, which are ignored otherwise); bg_forward: (bs, bg_dim, is, is) NCHW -> (bs, 3, is, is), fp32. */
LWG_API int lwg_generator_enable_bg(lwg_generator *g, int bg_dim);
LWG_API int lwg_generator_bg_forward(lwg_generator *g, const float *bg_inputs_nchw, int bs, float *out_nchw,
                                     lwg_stream_t stream);

/* Feed one state_dict entry (PyTorch layout, HOST memory), e.g.
 * "tsf_model.encoders.0.0.weight" (64,6,7,7), "tsf_model.resnets.2.main.1.bias" (512,),
 * "tsf_model.decoders.0.0.weight" (512,256,3,3), "tsf_model.attetion_reg.0.weight" (1,64,7,7).
 * Keys of bg_model.* are accepted and ignored (not on this path).  Unknown keys: LWG_ERR_INVALID_ARG. */
LWG_API int lwg_generator_load_weight(lwg_generator *g, const char *key, const float *data_host, const int64_t *shape,
                                      int ndim);
/* number of src_model/tsf_model entries still missing (0 = ready) */
LWG_API int lwg_generator_missing_weights(const lwg_generator *g);

/* Shapes of the 4 + repeat_num cached source feature maps, in the order
 * encoder_outs[0..3], resnet_outs[0..repeat_num-1] (generator.py:136-147). */
LWG_API int lwg_generator_num_src_features(const lwg_generator *g);
LWG_API int lwg_generator_src_feature_shape(const lwg_generator *g, int index, int *C, int *H, int *W);

/* ImpersonatorGenerator.encode_src (generator.py:213-214): src_inputs (1,src_dim,is,is) NCHW ->
 * feats_nhwc[i] (1,H,W,C) for every feature above (caller-allocated). */
LWG_API int lwg_generator_encode_src(lwg_generator *g, const float *src_inputs_nchw, float *const *feats_nhwc,
                                     lwg_stream_t stream);

/* ImpersonatorGenerator.inference (generator.py:277-301) + the blend of Imitator.forward
 * (models/imitator.py:326-336).
 *   tsf_inputs: layout 0 = NCHW (bs,tsf_dim,is,is); 1 = NHWC8 (bs,is,is,8)
 *   T (bs,is,is,2); feats_nhwc as produced by encode_src (batch 1, shared by all frames)
 *   color (bs,3,is,is), mask (bs,1,is,is): may be NULL
 *   bg (bg_bs,3,is,is) with bg_bs in {1,bs} and pred (bs,3,is,is) = mask*bg + (1-mask)*color: both may be NULL
 */
LWG_API int lwg_generator_inference(lwg_generator *g, const float *tsf_inputs, int layout, const float *T, int bs,
                                    const float *const *feats_nhwc, int align_corners, float *color, float *mask,
                                    const float *bg, int bg_bs, float *pred, lwg_stream_t stream);

/* ImpersonatorGenerator.swap (generator.py:245-275): two warped sources per level; optional fused blend
 * pred = mask*bg + (1-mask)*color of Swapper.forward (models/swapper.py:261-271), bg/pred as in inference. */
LWG_API int lwg_generator_swap(lwg_generator *g, const float *tsf_inputs, int layout, const float *T12,
                               const float *T21, int bs, const float *const *feats12_nhwc,
                               const float *const *feats21_nhwc, int align_corners, float *color, float *mask,
                               const float *bg, int bg_bs, float *pred, lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Background inpaintor: replaces what PyTorch dispatches for InpaintSANet(c_dim=4) in eval mode
 * (networks/inpaintor.py:110-202): 35 gated convolutions with folded BatchNorm, nearest x2 up-sampling,
 * one self-attention over (image_size/4)^2 tokens, mask compositing and clamps.  Runs once per source image
 * (models/imitator.py:124-125), batch 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lwg_inpaint lwg_inpaint;
LWG_API int lwg_inpaint_create(lwg_inpaint **out, int c_dim, int image_size);
LWG_API void lwg_inpaint_destroy(lwg_inpaint *g);
/* state_dict entries in PyTorch layout (HOST memory), e.g. "coarse_net.3.mask_conv2d.weight" (128,64,4,4),
 * "refine_upsample_net.2.conv2d.batch_norm2d.running_var" (64,), "refine_attn.gamma" (1,);
 * "...num_batches_tracked" is accepted and ignored. */
LWG_API int lwg_inpaint_load_weight(lwg_inpaint *g, const char *key, const float *data_host, const int64_t *shape,
                                    int ndim);
LWG_API int lwg_inpaint_missing_weights(const lwg_inpaint *g);
/* Arithmetic of the gated convolutions with >= 32 input channels (31 of the 35; the 5x5 entry layers, the 16 -> 3 exit layers and
 * the attention's projections and products always run in exact fp32): 1 (default) = bf16x3, the split-operand kernels of the
 * generator (three bf16 MFMA products per multiply-add, fp32 accumulate); 0 = exact fp32 MFMA everywhere. */
LWG_API int lwg_inpaint_set_precision(lwg_inpaint *g, int precision);
/* InpaintSANet.forward(imgs, masks) (inpaintor.py:178-202): imgs (1,3,is,is), masks (1,1,is,is) ->
 * coarse_x [optional], x (refined, clamped), comp_imgs = x*masks + imgs*(1-masks) [optional], all (1,3,is,is). */
LWG_API int lwg_inpaint_forward(lwg_inpaint *g, const float *imgs, const float *masks, float *coarse_x, float *x,
                                float *comp_imgs, lwg_stream_t stream);
/* Diagnostic entry (as lwg_generator_peek: for tests, not a hot path): the inpaintor's self-attention alone, through the launch
 * code lwg_inpaint_forward runs.  out = gamma * softmax((q + b_q)(k + b_k)^T)(v + b_v) + x over N tokens; qkv (N,192): the raw
 * 1x1-conv output [q 16 | k 16 | v 128 | 32 unused] per token, bias (192) laid out alike, x and out (N,128); all device, 16-byte
 * aligned.  kernel 0: the streaming vector-ALU kernel (N % 64 == 0).  kernel 1: the matrix-core kernel over key_chunks chunks
 * of whole 32-key tiles plus the merge (N % 256 == 0, N % (32 key_chunks) == 0); key_chunks 0 = what lwg_inpaint_create picks
 * for N.  split_out 1 (kernel 1 only): out in the split-bf16 format, per 32 channels [32 bf16 hi | 32 bf16 lo].  workspace
 * (kernel 1): lwg_inpaint_attention_workspace_bytes, scratch only; kernel 0 takes NULL / 0. */
LWG_API size_t lwg_inpaint_attention_workspace_bytes(int N, int kernel, int key_chunks);
LWG_API int lwg_inpaint_attention(const float *qkv, const float *bias, const float *x, float gamma, int N, int kernel,
                                  int key_chunks, int split_out, float *out, void *workspace, size_t workspace_bytes,
                                  lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * HMR regressor: replaces what PyTorch dispatches for HumanModelRecovery.forward (networks/hmr.py:119-300) in eval mode:
 * a pre-activation ResNet-50 (53 convolutions, BatchNorm on running statistics, max pool, average pool) and the
 * 3-iteration ThetaRegressor.  Exact fp32 (v_mfma_f32_32x32x2_f32); NHWC activations with the pixel dimension flattened
 * across images, so every row of a batch is bit-identical to the same image run alone, whatever max_batch is.
 * One stream, no host synchronisation, no allocation after create: a forward can be captured in a HIP graph.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lwg_hmr lwg_hmr;
/* num_blocks: bottleneck blocks per layer (hmr.py:176-177), NULL = {3,4,6,3}.  Scratch for batches up to max_batch. */
LWG_API int lwg_hmr_create(lwg_hmr **out, int max_batch, const int *num_blocks);
LWG_API void lwg_hmr_destroy(lwg_hmr *h);
/* The weights as ONE packed fp32 blob (HOST memory) of lwg_hmr_weight_floats() floats, everything laid out for the kernels and
 * BatchNorm folded to scale = gamma / sqrt(var + 1e-5), shift = beta - mean * scale by the caller (in fp64, rounded once;
 * impersonator_amd/networks/hmr.py::pack_weights is the one writer).  Order:
 *   stem w (7,7,3,64) [kh][kw][ci][co] | stem bias (64)
 *   per block: bn1 scale, shift (Cin) | conv1 w (Cin,p) | bn2 scale, shift (p) | conv2 w (3,3,p,p) | bn3 scale, shift (p)
 *              | conv3 w (p,4p) | conv3 bias (4p) | when Cin != 4p: shortcut w (Cin,4p) | shortcut bias (4p)
 *   post_bn scale, shift (2048) | mean_theta (85) | fc1 w (1024,2133), b | fc2 w (1024,1024), b | fc3 w (85,1024), b
 * Synchronises the device (the blob is replaced under no running forward). */
LWG_API size_t lwg_hmr_weight_floats(const lwg_hmr *h);
LWG_API int lwg_hmr_set_weights(lwg_hmr *h, const float *blob_host, size_t n_floats);
/* images (n,3,height,width) NCHW in [-1,1], height = width = 224 (anything else: LWG_ERR_UNSUPPORTED), n <= max_batch
 * -> theta_out (n,85) = [cam 3 | pose 72 | shape 10]; features_out (n,2048) or NULL. */
LWG_API int lwg_hmr_forward(lwg_hmr *h, const float *images, int n, int height, int width, float *theta_out,
                            float *features_out, lwg_stream_t stream);
/* Op-level entry points (what lwg_hmr_forward is made of; the tests call them directly).
 * conv: x (N,H,W,Cin) NHWC, w (k,k,Cin,Cout) [kh][kw][ci][co] -> y (N,Ho,Wo,Cout); (k,stride,pad) one of (1,1,0) (3,1,1) (3,2,1)
 *   (7,2,3); Cout a multiple of 64; any N, H, W >= 1.  All optional (NULL): prologue x <- max(x*pre_scale[ci] + pre_shift[ci], 0) on
 *   the input (padding stays 0); epilogue v + bias[co], then max(v*post_scale[co] + post_shift[co], 0), then + residual[n, oh*res_stride,
 *   ow*res_stride, co] of an NHWC tensor (N,res_H,res_W,Cout).  Pointers 16-byte aligned.
 * maxpool: F.max_pool2d(kernel 3, stride 2, ceil_mode=True), no padding: (N,H,W,C) -> (N,ceil((H-3)/2)+1,ceil((W-3)/2)+1,C); C % 4 == 0.
 * pool_features: out (N,C) = mean over the HW pixels of max(x*scale + shift, 0); x (N,HW,C).
 * regress: ThetaRegressor.forward (hmr.py:239-252): features (N,2048), weights in PyTorch layout on the DEVICE -> theta_out (N,85);
 *   workspace: lwg_hmr_regress_workspace_bytes(N), scratch only. */
LWG_API int lwg_hmr_conv(const float *x, int N, int H, int W, int Cin, const float *w, int Cout, int k, int stride, int pad,
                         const float *pre_scale, const float *pre_shift, const float *bias, const float *post_scale,
                         const float *post_shift, const float *residual, int res_stride, int res_H, int res_W, float *y,
                         lwg_stream_t stream);
LWG_API int lwg_hmr_maxpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream);
LWG_API int lwg_hmr_pool_features(const float *x, int N, int HW, int C, const float *scale, const float *shift, float *out,
                                  lwg_stream_t stream);
LWG_API size_t lwg_hmr_regress_workspace_bytes(int N);
LWG_API int lwg_hmr_regress(const float *features, int N, const float *mean_theta, const float *fc1_w, const float *fc1_b,
                            const float *fc2_w, const float *fc2_b, const float *fc3_w, const float *fc3_b, float *theta_out,
                            void *workspace, size_t workspace_bytes, lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LPIPS (csrc/lpips.hip): the reference's PerceptualMetric -- PerceptualLoss(model='net-lin', net='alex'), version 0.1
 * (thirdparty/his_evaluators/.../metrics/lpips: PNetLin.forward) in eval mode -- for the paired evaluator: pred and ref frames in,
 * one FP64 distance per frame out, no float frame taken to the host.
 * The network is torchvision's alexnet().features[0:12]: conv 3->64 k11 s4 p2 | ReLU | MaxPool(3,2) | conv 64->192 k5 p2 | ReLU |
 * MaxPool(3,2) | conv 192->384 k3 p1 | ReLU | conv 384->256 k3 p1 | ReLU | conv 256->256 k3 p1 | ReLU, tapped after each ReLU.
 * Exact fp32 convolutions (v_mfma_f32_32x32x2_f32, K = (tap, ci) ascending), NHWC activations, pred and ref as ONE batch of 2n
 * images; per tap and frame, in fp64 from the fp32 features: s_i = sum_c x_i,c^2, n_i = sqrt(s_i) + 1e-10,
 * d = sum_c w_c (x_0,c/n_0 - x_1,c/n_1)^2, the mean of d over the pixels; the frame's distance is the sum of its five taps in tap
 * order.  Fixed reduction orders, no atomics: a frame's numbers are the same bits at any batch size, at any position in the
 * batch, and with pred and ref swapped.  One stream, no host synchronisation, no allocation after create: a forward can be
 * captured in a HIP graph as one chain of launches.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lwg_lpips lwg_lpips;
/* Scratch for 2 * max_pairs images of up to max_h x max_w (both >= 31) is allocated here. */
LWG_API int lwg_lpips_create(lwg_lpips **out, int max_pairs, int max_h, int max_w);
LWG_API void lwg_lpips_destroy(lwg_lpips *h);
/* The weights as ONE packed fp32 blob (HOST memory) of lwg_lpips_weight_floats() floats
 * (impersonator_amd/networks/lpips.py::pack_weights is the one writer).  Order:
 *   per conv: w (k,k,Cin,Cout) [kh][kw][ci][co] | bias (Cout);  then the five lin vectors (64, 192, 384, 256, 256).
 * Synchronises the device (the blob is replaced under no running forward). */
LWG_API size_t lwg_lpips_weight_floats(const lwg_lpips *h);
LWG_API int lwg_lpips_set_weights(lwg_lpips *h, const float *blob_host, size_t n_floats);
/* pred, ref (n,3,H,W) fp32 NCHW -> dist (n) FP64, taps (n,5) FP64 or NULL.  mode: the pixel modes 0, 1, 2 of lwg_eval_pair_stats,
 * applied to both images in front of LPIPS's scaling layer (x - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448,
 * .450), every step a separately rounded fp32 operation; zero padding applies after the scaling.
 * H or W < 31 (31 -> 7 -> 3 -> 1: the smallest size at which relu5 still has a pixel): LWG_ERR_UNSUPPORTED; n > max_pairs, H > max_h,
 * W > max_w or no weights set: LWG_ERR_STATE; a mode outside 0..2: LWG_ERR_INVALID_ARG. */
LWG_API int lwg_lpips_forward(lwg_lpips *h, const float *pred, const float *ref, int n, int H, int W, int mode, double *dist,
                              double *taps, lwg_stream_t stream);
/* Op-level entry points (what lwg_lpips_forward is made of; the tests call them directly).  Every argument is checked before the
 * first HIP call.
 * conv: w (k,k,Cin,Cout) [kh][kw][ci][co], bias (Cout) or NULL -> y (N,Ho,Wo,Cout) NHWC; (k,stride,pad) one of (11,4,2) (5,1,2)
 *   (3,1,1), Cout a multiple of 64 (else LWG_ERR_UNSUPPORTED); relu 0 / 1.  input_mode < 0: x is (N,H,W,Cin) NHWC as it is;
 *   0..2: x is (N,3,H,W) NCHW and the pixel mode + scaling prologue applies.  w 16-byte aligned, and x when NHWC with Cin % 4 == 0.
 * maxpool: F.max_pool2d(kernel 3, stride 2), floor mode, no padding: (N,H,W,C) -> (N,(H-3)/2+1,(W-3)/2+1,C); C % 4 == 0, H, W >= 3.
 * layer_distance: f0, f1 (n,P,C) NHWC feature blocks, w (C) -> out (n) FP64, one tap's term as stated above; C % 4 == 0. */
LWG_API int lwg_lpips_conv(const float *x, int N, int H, int W, int Cin, const float *w, const float *bias, int Cout, int k,
                           int stride, int pad, int relu, int input_mode, float *y, lwg_stream_t stream);
LWG_API int lwg_lpips_maxpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream);
LWG_API int lwg_lpips_layer_distance(const float *f0, const float *f1, int n, int P, int C, const float *w, double *out,
                                     lwg_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * InceptionV3 features (csrc/inception.hip) for the set metrics FID and Inception Score: the reference's
 * InceptionV3(output_blocks=[3], resize_input=False, normalize_input=False) (thirdparty/his_evaluators/.../metrics/metrics.py:16-158,
 * registered at 197-205) -- torchvision's inception_v3 in eval mode cut at the final average pool, `transform_input`, AuxLogits and
 * fc never run -- behind the preprocessing of FIDMetric / InceptionScoreMetric (metrics.py:645-669, 715-740): `out *= 2; out -= 1`,
 * then F.interpolate(out, (299,299), 'bilinear', align_corners=False).  Frames in, 2048 fp32 features per frame out.
 * 94 x (Conv2d(bias=False) + BatchNorm2d(eps=1e-3) + ReLU) as exact fp32 convolutions (v_mfma_f32_32x32x2_f32, K = (kh, kw, ci)
 * ascending) over NHWC activations with the BatchNorm folded into a per-channel fmaf(acc, scale, shift); MaxPool(3,2) floor mode;
 * avg_pool2d(3,1,1) dividing by 9 everywhere; the global mean added in ascending pixel order in fp64 and rounded once.  The branches
 * of a Mixed block write their channel slices of the block's output themselves.  Fixed reduction orders, no atomics: a frame's
 * features are the same bits at any batch size and at any position in the batch.  One stream, no host synchronisation, no
 * allocation after create: a forward can be captured in a HIP graph as one chain of launches.
 * ---------------------------------------------------------------------------------------------- */
typedef struct lwg_inception lwg_inception;
/* Scratch for max_images frames of up to max_h x max_w -- taken as they are or resized to 299 x 299 -- is allocated here. */
LWG_API int lwg_inception_create(lwg_inception **out, int max_images, int max_h, int max_w);
LWG_API void lwg_inception_destroy(lwg_inception *h);
/* The weights as ONE packed fp32 blob (HOST memory) of lwg_inception_weight_floats() floats
 * (impersonator_amd/networks/inception.py::pack_weights is the one writer).  Per convolution, in torchvision's definition order
 * (Conv2d_1a_3x3 ... Mixed_7c.branch_pool): w (kh,kw,Cin,Cout) [kh][kw][ci][co] | scale (Cout) | shift (Cout), where
 * scale = gamma / sqrt(running_var + 1e-3) and shift = beta - running_mean * scale, computed in fp64 and rounded once.
 * Synchronises the device (the blob is replaced under no running forward). */
LWG_API size_t lwg_inception_weight_floats(void);
LWG_API int lwg_inception_set_weights(lwg_inception *h, const float *blob_host, size_t n_floats);
/* frames (n,3,H,W) fp32 NCHW -> features (n,2048) fp32.  mode: the pixel modes 0, 1, 2 of lwg_eval_pair_stats (1 is the
 * reference's `out *= 2; out -= 1` on [0,1] frames), applied before the resize.  (out_h, out_w): (299, 299) resizes bilinearly with
 * align_corners=False; (0, 0) feeds the frames as they are (the network is fully convolutional; its input must be at least 75 x 75).
 * tap_stage: -1, or one of the 18 stages 0..17 = Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3, the first max pool, Conv2d_3b_1x1,
 * Conv2d_4a_3x3, the second max pool, Mixed_5b, 5c, 5d, 6a, 6b, 6c, 6d, 6e, 7a, 7b, 7c (the map the global pool reads), whose NHWC
 * output (n,Hs,Ws,Cs) is copied to tap_out.
 * A network input below 75 x 75: LWG_ERR_UNSUPPORTED; n > max_images, H > max_h, W > max_w or no weights set: LWG_ERR_STATE; a mode
 * outside 0..2, another resize target, a tap_stage outside -1..17: LWG_ERR_INVALID_ARG. */
LWG_API int lwg_inception_forward(lwg_inception *h, const float *frames, int n, int H, int W, int mode, int out_h, int out_w,
                                  float *features, int tap_stage, float *tap_out, lwg_stream_t stream);
/* Op-level entry points (what lwg_inception_forward is made of; the tests call them directly).  Every argument is checked before
 * the first HIP call.
 * conv (BasicConv2d, torchvision/models/inception.py): w (kh,kw,Cin,Cout) [kh][kw][ci][co]; scale, shift (Cout) or NULL (1 and 0);
 *   y = relu?(fmaf(conv(x, w), scale, shift)) written to channels y_offset .. y_offset + Cout - 1 of the (N,Ho,Wo,y_pitch) NHWC
 *   buffer y, the other channels untouched.  kh, kw in 1..11, one stride 1..4, ph < kh and pw < kw, all independent; Cout a
 *   multiple of 4 (else LWG_ERR_UNSUPPORTED).  input_mode < 0: x is (N,H,W,Cin) NHWC as it is, Cin a multiple of 4 (else
 *   LWG_ERR_UNSUPPORTED), 16-byte aligned; 0..2: x is (N,3,H,W) NCHW frames in that pixel mode.  w 16-byte aligned.
 * maxpool: F.max_pool2d(kernel 3, stride 2), floor mode, no padding: (N,H,W,C) -> channels y_offset.. of (N,(H-3)/2+1,(W-3)/2+1,
 *   y_pitch); C, y_pitch and y_offset multiples of 4, H, W >= 3.
 * avgpool: F.avg_pool2d(kernel 3, stride 1, padding 1), count_include_pad=True: (N,H,W,C) -> (N,H,W,C); C a multiple of 4.
 * global_pool: F.adaptive_avg_pool2d(x, 1): (N,P,C) -> (N,C), P = H*W pixels added in ascending order in fp64, rounded once. */
LWG_API int lwg_inception_conv(const float *x, int N, int H, int W, int Cin, const float *w, const float *scale, const float *shift,
                               int Cout, int kh, int kw, int stride, int ph, int pw, int relu, int input_mode, float *y, int y_pitch,
                               int y_offset, lwg_stream_t stream);
LWG_API int lwg_inception_maxpool(const float *x, int N, int H, int W, int C, float *y, int y_pitch, int y_offset,
                                  lwg_stream_t stream);
LWG_API int lwg_inception_avgpool(const float *x, int N, int H, int W, int C, float *y, lwg_stream_t stream);
LWG_API int lwg_inception_global_pool(const float *x, int N, int P, int C, float *y, lwg_stream_t stream);

/* ---- training, first slice: the PatchGAN discriminator update ---------------------------------
 * Replaces PatchDiscriminator.forward (networks/discriminator.py:8-57, norm_type='instance', use_sigmoid=False) and,
 * for the discriminator, ImpersonatorTrainer._optimize_D + loss.backward() + torch.optim.Adam.step()
 * (models/impersonator_trainer.py:229-232, 396-414).  state_dict keys: "model.<i>.weight" (Cout,Cin,4,4) and
 * "model.<i>.bias" (Cout,) with the nn.Sequential indices of the reference (0, 2, 5, 8, ...). */
typedef struct lwg_discriminator lwg_discriminator;
LWG_API int lwg_discriminator_create(lwg_discriminator **out, int input_nc, int ndf, int n_layers, int image_size,
                                     int max_batch);
LWG_API void lwg_discriminator_destroy(lwg_discriminator *d);
LWG_API int lwg_discriminator_load_weight(lwg_discriminator *d, const char *key, const float *data_host,
                                          const int64_t *shape, int ndim);
/* copies a parameter (from_grads = 0) or its gradient (1) back to the host in PyTorch layout; synchronises */
LWG_API int lwg_discriminator_read_weight(lwg_discriminator *d, const char *key, int from_grads, float *data_host,
                                          size_t n_floats);
LWG_API int lwg_discriminator_num_params(const lwg_discriminator *d, size_t *n_floats);
/* Arithmetic of the discriminator's convolutions (forward, data gradient, weight gradient): 0 (default) fp32 MFMA; 1 bf16x3 --
 * the same fp32 tensors in memory, every operand split into two bf16 terms inside the kernels (hi*hi + hi*lo + lo*hi with
 * fp32 accumulation, ~2^-16 relative per product), what `conv_precision='bf16x3'` selects for the generator's streams
 * (reference: networks/discriminator.py:8-57 run in fp32 by cuDNN; the training step's tolerance is a loss curve, not bits). */
LWG_API int lwg_discriminator_set_precision(lwg_discriminator *d, int mode);
LWG_API int lwg_discriminator_output_size(const lwg_discriminator *d, int *h);   /* patch map edge (14 at 256, n_layers 4) */
/* x (bs,input_nc,is,is) NCHW device -> out (bs,1,h,h) */
LWG_API int lwg_discriminator_forward(lwg_discriminator *d, const float *x_nchw, int bs, float *out, lwg_stream_t stream);
/* loss = mean((D(real)-1)^2) + mean((D(fake)+1)^2) and its gradient wrt every parameter, into the handle's flat
 * gradient buffer (real, fake: (bs,input_nc,is,is) NCHW device; loss_device: optional device float). */
LWG_API int lwg_discriminator_backward(lwg_discriminator *d, const float *real_nchw, const float *fake_nchw, int bs,
                                       float *loss_device, lwg_stream_t stream);
/* The flat device buffers (n_floats each, identical layout): what a data-parallel job all-reduces between backward
 * and adam_step (torch.distributed / RCCL on the caller's side; padding entries are always zero). */
LWG_API int lwg_discriminator_buffers(lwg_discriminator *d, float **params, float **grads, size_t *n_floats);
/* torch.optim.Adam(lr, betas=(beta1, beta2), eps) step on the gradient buffer */
LWG_API int lwg_discriminator_adam_step(lwg_discriminator *d, float lr, float beta1, float beta2, float eps,
                                        lwg_stream_t stream);

/* ---- op-level convolution and its gradients (building blocks of the generator-side training step) ----------------
 * Tensors NHWC fp32 on the device; weights in PyTorch layout: (Cout,Cin,k,k) for Conv2d, (Cin,Cout,3,3) for
 * ConvTranspose2d(k3,s2,p1,output_padding 1) (`transposed` = 1; H, W are then the INPUT size, the output is 2H x 2W).
 * Replaces F.conv2d / F.conv_transpose2d and torch.autograd's conv backward (the reference: networks/generator.py:8-20,
 * 80-133 under loss.backward(), models/impersonator_trainer.py:355-357).  fp32 MFMA; channel counts powers of two >= 8,
 * the side that becomes the GEMM's N dimension a multiple of 64 (Cout for forward, Cin for backward_data; for
 * backward_weight Cout, or Cin when transposed).  stride 1: any k <= 7 with 'same' padding for backward_data;
 * stride 2: k3 p1 on even sizes.  workspace: lwg_conv2d_workspace_bytes, scratch only (nothing persists).
 * precision 0: fp32 MFMA.  precision 1 (bf16x3: operands carried as two bf16 terms, three MFMA products, fp32
 * accumulation: ~2^-16 relative per operand): forward and backward_data run the inference path's kernel wherever the
 * layer fits it -- no bias, reduction-side channels a multiple of 32, output grid per image a multiple of 128 pixels, at
 * most 32 taps -- and the fp32 kernel elsewhere; backward_weight runs its own bf16x3 kernel on every layer.
 * backward_data has one few-channel case besides: stride 1, k 7, pad 3, Cin == 8, Cout % 64 == 0 -- the data gradient of the
 * 7x7 stems (networks/generator.py:84: dy (N,H,W,Cout), w (Cout,8,7,7) -> dx (N,H,W,8)), which a second pass fed with the
 * first pass's image needs (models/imitator.py:384-406).  It runs a vector-ALU kernel of its own (not the implicit GEMM,
 * which would pad the 8 outputs to 64): exact fp32 FMAs in a fixed order WHATEVER `precision` says -- precision 1 gives the
 * same bits as precision 0 -- no atomics, bit-reproducible.  N <= 65535.  Its scratch, the flipped and transposed filter
 * (Cin * Cout * 49 floats), is inside lwg_conv2d_workspace_bytes. */
typedef struct lwg_conv2d_desc {
    int N, H, W, Cin, Cout, k, stride, pad, transposed;
    int precision;
} lwg_conv2d_desc;
LWG_API size_t lwg_conv2d_workspace_bytes(const lwg_conv2d_desc *d);
LWG_API int lwg_conv2d_forward(const lwg_conv2d_desc *d, const float *x, const float *w, const float *bias, float *y,
                               void *workspace, size_t workspace_bytes, lwg_stream_t stream);
LWG_API int lwg_conv2d_backward_data(const lwg_conv2d_desc *d, const float *dy, const float *w, float *dx,
                                     void *workspace, size_t workspace_bytes, lwg_stream_t stream);
LWG_API int lwg_conv2d_backward_weight(const lwg_conv2d_desc *d, const float *x, const float *dy, float *dw, float *dbias,
                                       void *workspace, size_t workspace_bytes, lwg_stream_t stream);

/* The regression heads inside the training step (networks/generator.py:142-152, 163-171: img_reg = Conv2d(64,3,7,1,3) +
 * Tanh, attetion_reg = Conv2d(64,1,7,1,3) + Sigmoid, no bias).  x (N,H,W,64) NHWC; w (w_rows >= 4, 64, 7, 7): rows 0-2 the
 * colour head, row 3 the mask head.  forward: color (N,3,H,W) = tanh(conv), mask (N,1,H,W) = sigmoid(conv), either may
 * be NULL.  backward_weight: dy8 (N,H,W,8) = gradient wrt the PRE-activation outputs (channels 4-7 zero) -> dw (8,64,7,7).
 * The data gradient is lwg_conv2d_backward_data with Cout = 8.  workspace: lwg_heads_workspace_bytes, scratch only.
 * PRECONDITION: x >= 0 (it is the output of the last IN + ReLU block, generator.py:129-133,178-181).  The forward is the
 * inference path's heads kernel, whose operand load folds that ReLU in: a negative entry of x is read as 0, i.e. the
 * entry point computes tanh/sigmoid(conv(max(x, 0))) and neither gradient accounts for the clamp. */
LWG_API size_t lwg_heads_workspace_bytes(int N, int H, int W);
LWG_API int lwg_heads_forward(const float *x, int N, int H, int W, const float *w, int w_rows, float *color, float *mask,
                              void *workspace, size_t workspace_bytes, lwg_stream_t stream);
LWG_API int lwg_heads_backward_weight(const float *x, const float *dy8, int N, int H, int W, float *dw, void *workspace,
                                      size_t workspace_bytes, lwg_stream_t stream);

/* Diagnostic entries (as lwg_inpaint_attention: for tests, not a hot path): the two direct kernels of the default bf16x3 inference
 * path on their own, through the launch code lwg_generator_inference runs, so that they can be held against float64 at shapes the
 * whole generator never gives them.  Every argument is checked before the first HIP call.
 *
 * lwg_stem_forward: the generator's first layer, Conv2d(cin -> 64, k7, s1, p3, no bias), on an NHWC8 input.
 *   x (N,H,W,8) fp32, 16-byte aligned; channels cin..7 are never read as data (channels 6-7 not at all; cin..5 meet zero weights),
 *     but EVERY value of channels 0..5 must be finite: the padded tail of a 48-entry run multiplies the next pixel's channels by
 *     zero weights, so a NaN / Inf pixel reaches outputs outside its 7x7 footprint (precision 1);
 *   w_host (64,cin,7,7) in HOST memory, PyTorch layout, 1 <= cin <= 6: packed and uploaded as lwg_generator_load_weight does;
 *   precision 1: stem_bf16x3_kernel (W % 128 == 0, H % 2 == 0, else LWG_ERR_UNSUPPORTED); precision 0: the exact-fp32 small-Cin
 *     implicit GEMM on the same arguments -- what the generator runs under lwg_generator_set_precision(g, 0);
 *   y (N,H,W,64) raw (pre-norm) output; partials (N*H*W/128, 64, 2) or NULL: (mean, M2) of y per channel over each run of 128
 *     consecutive pixels, the InstanceNorm statistics the generator reduces further;
 *   max_workgroups: 0 = the launcher's grid (one persistent workgroup per CU, at most one per two tiles), what the generator uses;
 *     > 0 caps it, so that a small tensor gives each four-wave group several tiles.  The schedule changes no result bit.
 *   Allocates and frees the device copy of the weights and synchronises the stream: not for a captured graph.
 *
 * lwg_heads_inference: tanh / sigmoid of Conv2d(64 -> 3 + 1, k7, p3, no bias) on relu(x * scale + shift), zero padding applied
 *   AFTER the normalisation (a padded tap contributes 0, not relu(shift)), plus the blend of Imitator.forward.
 *   x (N,H,W,64) raw fp32, 16-byte aligned; scale_shift (N,64,2) = (scale, shift) per image and channel; w (w_rows >= 4,64,7,7) on
 *     the DEVICE, rows 0-2 colour, row 3 mask, further rows ignored; any N, H, W >= 1;
 *   precision 0: heads_kernel (exact fp32, vector ALU); 1: heads_bf16x3_kernel (matrix cores, hardware exp / rcp activations);
 *   bg (bg_bs,3,H,W) with bg_bs in {1, N} or NULL; outputs, each optional but one required: color (N,3,H,W), mask (N,1,H,W),
 *     pred (N,3,H,W) = mask*bg + (1-mask)*color (needs bg);
 *   bands (precision 1 only): 0 = the launcher's choice of row bands per 26-column strip from the CU count, what the generator
 *     uses; > 0 forces min(bands, H) bands of ceil(H / bands) rows.  An output row's bits do not depend on the banding.
 *   workspace: lwg_heads_inference_workspace_bytes, 16-byte aligned, scratch only.  Enqueued on the stream, no synchronisation. */
LWG_API int lwg_stem_forward(const float *x, int N, int H, int W, const float *w_host, int cin, int precision, float *y,
                             float *partials, int max_workgroups, lwg_stream_t stream);
LWG_API size_t lwg_heads_inference_workspace_bytes(int N, int H, int W);
LWG_API int lwg_heads_inference(const float *x, int N, int H, int W, const float *scale_shift, const float *w, int w_rows,
                                int precision, const float *bg, int bg_bs, float *color, float *mask, float *pred, int bands,
                                void *workspace, size_t workspace_bytes, lwg_stream_t stream);

/* Diagnostic entries (as lwg_stem_forward: for tests, not a hot path): the inference path's norm chain, link by link.  Every layer
 * of lwg_generator_inference is conv -> per-tile (mean, M2) written by the conv's epilogue -> finalize -> apply (or, where the
 * consumer is a halo kernel, the apply folded into that consumer's operand load).  Each link runs here on caller-supplied tensors
 * through the launch code the generator runs.  Every argument is checked before the first HIP call.
 *
 * lwg_norm_conv_forward: one layer as the generator launches it -- the non-general kernels with their statistics epilogue.
 *   d: precision 0 (exact fp32) or 1 (bf16x3), transposed 0 or 1; x (N,H,W,Cin) plain fp32 NHWC; w in PyTorch layout (as
 *     lwg_conv2d_forward); the entry re-lays the weights out, splits x (precision 1) and keeps the zero run behind it.
 *   The output grid per image (Hm x Wm: Ho x Wo, or H x W for a transposed conv, whose four output parities are four PHASES
 *     p = 2*py + px holding the pixels (2i+py, 2j+px)) must be a multiple of 128 pixels.
 *   bn: output channels per workgroup tile, 32 / 64 / 128 passed to the dispatcher as given; 0 = the generator's rule: 128 once
 *     Cout % 128 == 0 and the launch has >= 256 such tiles, else 64 (exact fp32 with few tiles: 32).  A transposed layer runs
 *     unfused on the 128-channel tile when precision 1 and Cout % 128 == 0, else as one workgroup walking all four phases of a
 *     64-channel tile, whatever bn says.  What the dispatcher refuses is returned with its code.
 *   y (N,Ho,Wo,Cout) raw output; partials (nphase, mtiles, Cout, 2), mtiles = N*Hm*Wm/128: (mean, M2 = sum of squared deviations
 *     from that mean) of y over 128 output pixels of one phase and channel.  WHICH 128 pixels partial t of phase p covers:
 *       - ring and fp32 kernels (conv_igemm_bf16x3, conv_igemm_dma_f32, conv_igemm_f32): pixels 128t .. 128t+127 of the phase's
 *         grid flattened as (image, hm, wm), images in order -- a run of 128 consecutive pixels; the 256-row ring tile writes
 *         the two runs 2u, 2u+1 of its workgroup u;
 *       - halo kernels (conv3x3_halo_bf16x3, plain and transposed): the 4-row x 32-column blocks of the Hm x Wm grid, numbered
 *         row-major within the image, images in order: t = image * (Hm/4)*(Wm/32) + (hm/4) * (Wm/32) + wm/32.  The tall (8 x 32)
 *         tile writes two of them: its upper block at that index and its lower block Wm/32 entries (one block row) further.
 *       At Wm == 32 the two numberings coincide.  Within a partial the 128 values are reduced as four groups of 32 (mean and M2
 *       each) combined by Chan's formula; the order inside a group is the kernel's own.
 *   variant_host (optional, HOST int): the kernel family that ran, an index for lwg_generator_profile_variant_name.
 *   in_scale_shift (optional, precision 1): (N, Cin - raw_from, 2) -- channels >= raw_from of x are then a producer's RAW output
 *     which the kernel normalises itself, relu(x * scale + shift) and the hi/lo split, zero padding applied AFTER it; raw_from a
 *     multiple of 32.  Only the halo kernels take it: LWG_ERR_UNSUPPORTED elsewhere.
 *   workspace: lwg_norm_conv_workspace_bytes, 16-byte aligned, scratch only.  Enqueued on the stream, no synchronisation.
 *
 * lwg_norm_finalize: partials (nphase, mtiles, C, 2) as above, mtiles = N * tiles per image -> scale_shift (N, C, 2) =
 *   (gamma * inv, beta - mean * gamma * inv), inv = 1 / sqrt(var + eps), var the BIASED variance of the image's nphase * mtiles/N
 *   * 128 samples: Chan's combination of the partials in double, rounded to fp32 once per output.
 *   Conditioning contract: the between-tile term is computed as sum(mean_t^2) - cnt * mean^2, which cancels when |mean| >> std.
 *   For |mean| / std <= 2^12 both outputs are within 2 fp32 ulp of the exactly combined value (CPU emulations of the kernel's
 *   arithmetic put the worst at 0.5 to 0.7 ulp); beyond, the error grows with the square of the ratio (1 to 6 ulp at 2^14, 12 to
 *   90 at 2^16, depending on the partials) -- there the fp32 rounding of shift itself, ~ratio * 2^-24 of a normalised unit, already
 *   exceeds what apply can deliver.  tests/test_gpu_norm_chain.py asserts the contract and prints the figures beyond it.
 *
 * lwg_norm_apply: dst = [relu](raw * scale + shift) [+ res] [+ sum_k grid_sample(warp_src_k, warp_T_k)] per pixel and channel.
 *   raw (N,H,W,C) dense fp32; scale_shift (N,C,2); dst: pixel stride ld_dst >= C floats (a channel slice of a wider buffer, offset
 *     already applied); res likewise with ld_res, or NULL; split 1: dst is written, and res read, in the split-bf16 format (per 32
 *     channels [32 bf16 hi | 32 bf16 lo]; C, strides % 32 == 0, 128-byte aligned), split 0: both fp32;
 *   nwarp 0..2 Liquid-Warping terms: warp_src_k (warp_n_k,H,W,C) fp32 with warp_n_k in {1 (shared), N}, warp_T_k (N,H,W,2) the
 *     flow, bilinear with zero padding as lwg_grid_sample_nhwc, added AFTER the activation in the order k = 0, 1;
 *   lanes: 0 = the launcher's choice, 4 = apply_kernel (four channels per thread), 8 = apply8_kernel (split only).  C % 4 == 0. */
LWG_API size_t lwg_norm_conv_workspace_bytes(const lwg_conv2d_desc *d);
LWG_API int lwg_norm_conv_forward(const lwg_conv2d_desc *d, const float *x, const float *w, int bn, const float *in_scale_shift,
                                  int raw_from, float *y, float *partials, int *variant_host, void *workspace,
                                  size_t workspace_bytes, lwg_stream_t stream);
LWG_API int lwg_norm_finalize(const float *partials, int nphase, int mtiles, int N, int C, const float *gamma, const float *beta,
                              float eps, float *scale_shift, lwg_stream_t stream);
LWG_API int lwg_norm_apply(const float *raw, int N, int H, int W, int C, const float *scale_shift, int relu, float *dst, int ld_dst,
                           const float *res, int ld_res, int split, int nwarp, const float *warp_src0, int warp_n0,
                           const float *warp_T0, const float *warp_src1, int warp_n1, const float *warp_T1, int align_corners,
                           int lanes, lwg_stream_t stream);

/* Generator-side adversarial term (models/impersonator_trainer.py:369-371): loss = mean((D(x) - target)^2) on
 * x (bs,input_nc,is,is) NCHW and its gradient wrt x (same shape); the discriminator's parameters get no gradient. */
LWG_API int lwg_discriminator_input_grad(lwg_discriminator *d, const float *x_nchw, int bs, float target, float *loss_device,
                                         float *dx_nchw, lwg_stream_t stream);
/* lwg_discriminator_backward and lwg_discriminator_input_grad with a factor on the loss: loss = loss_scale * (...), gradients
 * scaled with it at their source (the loss gradient on the patch map), nothing rescaled afterwards.  loss_scale = 1 gives the
 * unscaled entry points' bits.
 * GlobalLocalDiscriminator takes one mean over the concatenation of its two branches' patch maps (networks/discriminator.py:77,
 * models/impersonator_trainer_aug.py:380-381, 412-425); both maps have one shape, so each branch runs with loss_scale = 0.5. */
LWG_API int lwg_discriminator_backward_scaled(lwg_discriminator *d, const float *real_nchw, const float *fake_nchw, int bs,
                                              float loss_scale, float *loss_device, lwg_stream_t stream);
LWG_API int lwg_discriminator_input_grad_scaled(lwg_discriminator *d, const float *x_nchw, int bs, float target,
                                                float loss_scale, float *loss_device, float *dx_nchw, lwg_stream_t stream);
/* bilinear grid_sample (zeros padding) on NHWC tensors: x (xn,H,W,C), xn in {1, n}; grid (n,Ho,Wo,2) -> y (n,Ho,Wo,C) */
LWG_API int lwg_grid_sample_nhwc(const float *x, int xn, int C, int H, int W, const float *grid, int n, int Ho, int Wo,
                                 int align_corners, float *y, lwg_stream_t stream);

/* InstanceNorm2d(affine=True, eps 1e-5, biased variance) [+ ReLU] and its gradient, NHWC fp32 (x: (N,HW,C)).
 * stats: (N,C,2) floats (mean, rstd) written by forward, read by backward.  backward: y = the forward output when it
 * went through the ReLU (its sign is the mask) or NULL; dgamma/dbeta (C,) overwritten.  scratch: device memory of
 * lwg_instance_norm_scratch_bytes(N, HW, C) bytes (8-byte aligned; slab partial sums of the two-stage reductions). */
LWG_API size_t lwg_instance_norm_scratch_bytes(int N, int HW, int C);
LWG_API int lwg_instance_norm_forward(const float *x, int N, int HW, int C, const float *gamma, const float *beta, int relu,
                                      float *y, float *stats, void *scratch, lwg_stream_t stream);
LWG_API int lwg_instance_norm_backward(const float *x, const float *y, const float *dy, const float *stats,
                                       const float *gamma, int N, int HW, int C, float *dx, float *dgamma, float *dbeta,
                                       void *scratch, lwg_stream_t stream);
/* Gradient of bilinear grid_sample (zeros padding) wrt its input, NHWC: dy (n,Ho,Wo,C), grid (n,Ho,Wo,2) ->
 * dx (xn,H,W,C) ACCUMULATED (zero it first), xn in {1, n}.  Atomic fp32 adds (not bit-reproducible, as torch's). */
LWG_API int lwg_grid_sample_backward(const float *dy, const float *grid, int xn, int C, int H, int W, int n, int Ho, int Wo,
                                     int align_corners, float *dx, lwg_stream_t stream);
/* The same gradient, DETERMINISTIC (what the training step uses; replaces torch's grid_sampler_2d_backward behind
 * networks/generator.py:312-315 in `loss_G.backward()`, models/impersonator_trainer.py:355-356): the scatter is planned once per
 * flow field -- every source texel gets the list of (output pixel, tap, bilinear weight) that reach it, sorted by pixel -- and
 * applied per tensor as a gather that adds the contributions in that fixed order (bit-reproducible; same zeros-padding taps and
 * weights as lwg_grid_sample_nhwc).  plan: caller-owned device memory of lwg_grid_sample_plan_bytes() bytes (4-byte aligned),
 * written by lwg_grid_sample_plan, read by any number of lwg_grid_sample_backward_planned calls with the SAME dimensions
 * (one plan serves every warp of a pyramid level: the Liquid Warping Block warps seven feature maps with one flow).
 * dx (xn,H,W,C) is ACCUMULATED (zero it first); C a multiple of 4. */
LWG_API size_t lwg_grid_sample_plan_bytes(int xn, int H, int W, int n, int Ho, int Wo);
LWG_API int lwg_grid_sample_plan(const float *grid, int xn, int H, int W, int n, int Ho, int Wo, int align_corners, void *plan,
                                 size_t plan_bytes, lwg_stream_t stream);
LWG_API int lwg_grid_sample_backward_planned(const float *dy, int C, int xn, int H, int W, int n, int Ho, int Wo, const void *plan,
                                             size_t plan_bytes, float *dx, lwg_stream_t stream);
/* torch.optim.Adam step (no weight decay, no amsgrad) on a flat fp32 device tensor; step counts from 1 */
LWG_API int lwg_adam_update(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, long step, float lr,
                            float beta1, float beta2, float eps, lwg_stream_t stream);
/* The same update with the step count in device memory: `step_state` is three 8-byte words on the device -- the count t
 * (int64) and beta1^t, beta2^t (doubles); {0, 1.0, 1.0} before the first step -- which the call advances on the stream (with the
 * betas it is given: keep them fixed) and then uses for the bias corrections.  Nothing about the step is baked into launch
 * arguments, so a captured HIP graph of a training iteration replays correctly. */
LWG_API int lwg_adam_update_device_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                                        void *step_state, float lr, float beta1, float beta2, float eps, lwg_stream_t stream);
/* The same again with the learning rate in device memory too: the update uses lr = lr_table[min(t, lr_count) - 1], t being the
 * count AFTER the advance (the first step reads entry 0; steps past the table keep its last entry).  lr_table: lr_count >= 1
 * floats on the device, read by the kernel when it runs -- neither step nor rate is a launch argument, so ONE captured graph
 * replays through a whole learning-rate schedule. */
LWG_API int lwg_adam_update_scheduled(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                                      void *step_state, const float *lr_table, int lr_count, float beta1, float beta2, float eps,
                                      lwg_stream_t stream);
/* lwg_discriminator_adam_step keeps its step count on the device as well (on != 0; synchronous, call outside a capture, with the
 * betas the following steps will use): see lwg_adam_update_device_step.  Switching it off copies the count back. */
LWG_API int lwg_discriminator_use_device_step(lwg_discriminator *d, int on, float beta1, float beta2);

/* Test hook: copies an internal scratch buffer (device to device) after inference/swap/encode_src.
 * which: 0..2 = concat buffers cat[l] (bs, is>>l, is>>l, 2*conv_dim<<l)  [skip half | decoder half],
 *        3 = residual trunk output (bs, is/8, is/8, 8*conv_dim), 4..5 = skipper outputs 0..1,
 *        6 = raw (pre-norm) output of the last conv, 7..9 = resized flows at is/2, is/4, is/8.
 * Copies min(n_floats, buffer size) floats. */
LWG_API int lwg_generator_peek(lwg_generator *g, int which, float *dst, size_t n_floats, lwg_stream_t stream);

/* Kernel timing for bench.py's roofline: when enabled, every launch of an implicit-GEMM conv kernel is bracketed by
 * HIP events on the launch stream.  The conv runs as one of lwg_generator_profile_variants() kernel instantiations
 * (names as rocprofv3 prints them: lwg_generator_profile_variant_name).  read() synchronises the events and returns,
 * for one variant (or all of them with variant = -1), the launch count, the summed duration and the algorithmic
 * FLOPs (2*M*N*K of the convolution with its real taps and channels; zero padding counted as cuDNN would count it,
 * the kernel's own K/channel padding not counted).  profile(enable) clears the record. */
LWG_API int lwg_generator_profile(lwg_generator *g, int enable);
LWG_API int lwg_generator_profile_variants(void);
LWG_API const char *lwg_generator_profile_variant_name(int variant);
LWG_API int lwg_generator_profile_read(lwg_generator *g, int variant, int *launches, double *total_ms,
                                       double *total_flops);

/* Measurement hook (tools/conv_trace.py; no reference counterpart -- rocprofv3's thread trace has no decoder in this
 * image): with a device buffer set, every launch of the dominant 128-channel bf16x3 conv kernel runs its instrumented
 * twin (same code + s_memtime reads around the stage's data wait and barrier) and appends one block of
 * [workgroup][wave][8] uint64 {start, loop start, loop end, end, cycles in the data wait, cycles in the barrier,
 * stages, hw id}.  trace_launch(i): {byte offset, grid x, y, z, waves, stages, Cin, Cout, Hm, N} of traced launch i, or
 * LWG_ERR_INVALID_ARG past the last one.  conv_trace(NULL, 0) switches it off.  Process-wide, not thread-safe. */
LWG_API int lwg_conv_trace(void *device_buffer, size_t bytes);
LWG_API int lwg_conv_trace_launch(int index, long long *info10);

/* Diagnostic (tests/test_wgrad_plan.py; no reference counterpart): what lwg_conv2d_backward_weight launches for `d` on a
 * device of cu_count compute units -- d is mapped to the weight-gradient shape as that entry point maps it (roles swapped
 * for a transposed conv), with part_floats floats for split-K partials (0: what that entry point carves from its workspace;
 * anything else as given, e.g. a discriminator's buffer).  info10: {route (0 3x3 row, 1 7x7 stem row, 2 per tap), row of the
 * kernel table, grid x, y, z, block, dynamic LDS bytes, pixel slices S, pixels per slice, reduction behind the kernel
 * (0 none, 1 reduce_slices4, 2 reduce_taps_direct, 3 reduce_taps)}.  The slice count fixes the order of summation, i.e. the
 * bits of the gradient.  Honours the process's LWG_WGRAD_ROW3 / LWG_WGRAD_ROW3_SLICES; every refusal of backward_weight's
 * dispatch is returned with its code.  No HIP call: needs no device. */
LWG_API int lwg_wgrad_plan(const lwg_conv2d_desc *d, size_t part_floats, int cu_count, long long *info10);

#ifdef __cplusplus
}
#endif
#endif /* LWG_H_ */
