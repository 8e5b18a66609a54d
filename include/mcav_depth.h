/* mcav_depth.h -- C ABI of libmcav_depth.so: the MI355X (gfx950) hot path of the self-supervised
 * depth+pose training step.  Plain pointers and sizes only; no torch types.
 *
 * The reference (Monash-Connected-Autonomous-Vehicle/unsupervised-pseuso-LiDAR) is pure Python/PyTorch and
 * has no FFI of its own: its "operator interface" for this path is the Python call surface
 * trainer.py:290-313 / losses.py:262-271 / geometry/pose_geometry.py:201-229 / models/.  Each entry point
 * below names the reference call it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (torch tensors' data_ptr()), fp32 unless noted;
 *   - image-like tensors at the API boundary are NCHW contiguous (the reference's layout);
 *     network-internal activations are NHWC (see mcav_conv.h section below);
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 on success, negative MCAV_E_* on error; nothing throws across the ABI;
 *   - stateless and thread-safe apart from the caller-provided workspace.
 */
#ifndef MCAV_DEPTH_H
#define MCAV_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCAV_OK 0
#define MCAV_E_INVALID (-1)   /* bad argument (null pointer, non-positive size, unsupported shape) */
#define MCAV_E_WORKSPACE (-2) /* workspace too small */
#define MCAV_E_LAUNCH (-3)    /* HIP launch/runtime error (hipGetLastError) */

/* ABI version of this header (bumped on any signature change). */
int mcav_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Loss stage (K10 + K11): fused inverse-warp -> bilinear sample -> L1 photometric -> second-order
 * smoothness, forward AND backward in one pass over the triplet.
 * Replaces Losses.forward (losses.py:262-271) = disp_to_depth (pose_geometry.py:70-95)
 *   + reprojection_loss (losses.py:183-240: 3 x inverse_warp (pose_geometry.py:201-229,
 *     transform.py:74-150, F.grid_sample) + nn.L1Loss) + smooth_loss(depths[0]) (losses.py:242-260)
 * and its autograd backward (trainer.py:264).
 *
 * flags */
#define MCAV_WL_K_F64 1u          /* intrinsics are fp64 [B,3,3] (as the reference's loader gives); else fp32 */
#define MCAV_WL_SKIP_IF_UNIT 2u   /* return without touching outputs when upstream[0]==upstream[1]==1 */
#define MCAV_WL_NO_SMOOTH 4u      /* leave the smoothness term out (used for scales > 0 of multi-scale nets) */
#define MCAV_WL_INPUT_DEPTH 8u    /* disp_t / disp_r0 already hold depths; gradients are w.r.t. depth */
#define MCAV_WL_SSIM 16u          /* photometric term = 0.85 * SSIM distance + 0.15 * L1 (reference losses.py:12-54, weights of :77) instead of L1 */
/* masked modes, mcav_warp_loss_masked_fwd_bwd only (the monodepth2 recipe, without its random noise on the identity error).  e_w(p): warp w's
 * per-pixel error (channel mean of the photometric term), i_w(p): the same error of its UNWARPED source against its target. */
#define MCAV_WL_MIN_REPROJ 32u    /* warps 0 and 1 (same target) become one term, mean_p min(e_0, e_1), of weight tw[0] + tw[1]; warp 2 unchanged */
#define MCAV_WL_AUTOMASK 64u      /* every term takes the minimum with its warps' identity errors: min(i_0, i_1, e_0, e_1) with MIN_REPROJ,
                                     else min(i_w, e_w) per warp.  A pixel won by an identity error adds it to the loss and has no gradient */

/* The workspace holds per-workgroup partial sums and the completion tickets of the fused kernel (since round 3 the per-sample constants and
 * the float64 finalize run INSIDE it: one launch).  It must be ZERO-FILLED before its first use; every launch leaves the tickets at zero, so
 * one buffer serves all later calls on the same stream.  One launch at a time per workspace. */
size_t mcav_warp_loss_workspace_bytes(int B, int H, int W);

/* tgt, ref0, ref1: [B,3,H,W].  disp_t, disp_r0: [B,1,H,W] sigmoid disparities of tgt and ref0 (scale 0).
 * poses: [B,2,6] (axis-angle, translation).  K: [B,3,3] fp64 or fp32 (flag).
 * upstream: 2 floats on the DEVICE = d(total)/d(loss_mam), d(total)/d(loss_smooth); NULL means (1,1).
 * term_weights: 3 floats on the HOST, weight of each warp's L1 mean inside loss_mam; NULL means
 *   (0.25, 0.25, 0.5) = the reference's single-scale combination (losses.py:227-240).
 * Outputs: losses[2] = (loss_mam, loss_smooth); d_disp_t, d_disp_r0: [B,1,H,W]; d_poses: [B,2,6]. */
int mcav_warp_loss_fwd_bwd(const float* tgt, const float* ref0, const float* ref1,
                           const float* disp_t, const float* disp_r0, const float* poses, const void* K,
                           int B, int H, int W, unsigned flags, const float* upstream, const float* term_weights,
                           float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                           void* workspace, size_t workspace_bytes, void* stream);

/* mcav_warp_loss_fwd_bwd with the masked modes: the same arguments and outputs, flags may add MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK.
 * Ties are deterministic: identity wins over reprojection on equality (a warp is kept only if e < i); among the identity errors and among
 * the reprojection errors warp 0 wins.  Only the selected reprojection receives gradient; a re-run on the same inputs selects the same.
 * selection: optional uint8 [B,2,H,W] on the DEVICE (NULL = not written; selection_bytes >= B*2*H*W):
 *   plane 0: the group of warps 0 and 1: 0 = warp 0, 1 = warp 1, 2 = identity.  Without MIN_REPROJ it holds warp 0's choice (0 = kept,
 *            2 = identity); warp 1's choice is not stored;
 *   plane 1: warp 2: 0 = kept, 2 = identity.
 * With neither new flag this is mcav_warp_loss_fwd_bwd (bit-identical results; the selection, if given, is zero-filled).
 * Returns MCAV_E_INVALID for unknown flag bits, MCAV_E_WORKSPACE for a selection buffer that is too small. */
int mcav_warp_loss_masked_fwd_bwd(const float* tgt, const float* ref0, const float* ref1,
                                  const float* disp_t, const float* disp_r0, const float* poses, const void* K,
                                  int B, int H, int W, unsigned flags, const float* upstream, const float* term_weights,
                                  float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                                  void* workspace, size_t workspace_bytes, void* stream,
                                  unsigned char* selection, size_t selection_bytes);

/* Mono + stereo ("MS", monodepth2): mcav_warp_loss_masked_fwd_bwd with one more source view, the stereo frame of the target, warped into the
 * target with depth(tgt), the same K and the FIXED transform [I | (-b, 0, 0)].  The known metric baseline b pins the scale of the depth (and
 * of the pose net's translations) to metres.  e_s / i_s: the stereo warp's error and the unwarped stereo frame's error against tgt.
 *   plain:                 loss_mam = tw0 mean e_0 + tw1 mean e_1 + tws mean e_s + tw2 mean e_2
 *   MIN_REPROJ:            (tw0 + tw1 + tws) mean_p min(e_0, e_1, e_s) + warp 2 as in the masked entry
 *   MIN_REPROJ + AUTOMASK: (tw0 + tw1 + tws) mean_p min(i_0, i_1, i_s, e_0, e_1, e_s) + tw2 mean_p min(i_2, e_2)
 *   AUTOMASK:              every warp, the stereo one included, takes min(i_w, e_w)
 * Ties continue the masked entry's order: identities (i_0, i_1, i_s), then reprojections (e_0, e_1, e_s); a later candidate wins only if
 * strictly smaller.  The stereo warp has no pose gradient; its gradient goes to disp_t only.  A pixel won by an identity sends none.
 * stereo: [B,3,H,W], the stereo frame (KITTI: image_03 for an image_02 target).
 * stereo_baseline: [B] float on the DEVICE (read by the kernel: a captured graph honours new values without a host sync), in metres: the x
 *   coordinate of the stereo camera's centre in the target camera's frame -- positive when the stereo camera is to the target's right
 *   (KITTI left target, right source: +0.54), negated for a horizontally mirrored sample.
 * term_weights: 4 floats on the HOST (tw0, tw1, tw2, tws); NULL means (1/6, 1/6, 1/2, 1/6): the target-view group is the mean of its three
 *   warps and warp 2 keeps its half.
 * selection: as in the masked entry; plane 0 gains code 3 = the stereo warp (codes 0, 1, 2 keep their meaning).  Without MIN_REPROJ plane 0
 *   holds warp 0's choice; without either masked flag it is zero-filled.
 * flags: MCAV_WL_K_F64 / SKIP_IF_UNIT / NO_SMOOTH / INPUT_DEPTH / SSIM / MIN_REPROJ / AUTOMASK.  Returns MCAV_E_INVALID for unknown flag bits
 * or a null pointer, MCAV_E_WORKSPACE for a workspace or selection buffer that is too small. */
int mcav_warp_loss_stereo_fwd_bwd(const float* tgt, const float* ref0, const float* ref1,
                                  const float* disp_t, const float* disp_r0, const float* poses, const void* K,
                                  int B, int H, int W, unsigned flags, const float* upstream, const float* term_weights,
                                  float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                                  void* workspace, size_t workspace_bytes, void* stream,
                                  unsigned char* selection, size_t selection_bytes,
                                  const float* stereo, const float* stereo_baseline);

/* Query, nothing is launched: the grid a launch of the fused L1 kernels would use.  Every sample gets G0 pass-0 and G1 pass-1 workgroups
 * (grid = (G0 + G1, B)); workgroup g of a pass walks the 32 x 16 pixel tiles g, g + G, ... of its sample.  The instantiation is the one the
 * entries above pick: the MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK bits of flags, and stereo != 0 for mcav_warp_loss_stereo_fwd_bwd's kernels.
 * slots > 0 plans for that many resident workgroups and needs no device; slots = 0 asks the runtime (CUs x workgroups per CU of that
 * instantiation) exactly as the launch does.  The launch and this query run one planner.
 * Returns MCAV_E_INVALID where the launch would (B <= 0, B > 4095, H < 3, W < 3, unknown flag bits), for a null G0 / G1 or slots < 0, and
 * for MCAV_WL_SSIM, whose kernels use one workgroup per tile. */
int mcav_warp_loss_l1_grid(int B, int H, int W, unsigned flags, int stereo, int slots, int* G0, int* G1);

/* DIAGNOSTIC twin of mcav_warp_loss_fwd_bwd (upstream (1,1)): the same kernel bodies with a per-pixel dump, used by
 * tests/flip_finder.py to NAME the pixels at which an fp32 evaluation takes another bilinear cell / L1 sign than float64 does
 * (losses.py:183-240 is only piecewise smooth).  taps: [B][3 warps][7][H][W] = { ix, iy (un-normalised sampling position, source pixels),
 * d loss_mam / d ix, d loss_mam / d iy, residual of channel 0..2 } per warp (0: ref0 -> tgt, 1: ref1 -> tgt, 2: tgt with depth(ref0) and the
 * inverted pose[0]; with MCAV_WL_SSIM the residual planes are left zero).  Not used by the training path. */
int mcav_warp_loss_debug_taps(const float* tgt, const float* ref0, const float* ref1,
                              const float* disp_t, const float* disp_r0, const float* poses, const void* K,
                              int B, int H, int W, unsigned flags, const float* term_weights,
                              float* losses, float* d_disp_t, float* d_disp_r0, float* d_poses,
                              void* workspace, size_t workspace_bytes, float* taps, size_t taps_floats, void* stream);

/* Standalone inverse_warp (pose_geometry.py:201-229): img [B,3,H,W], depth [B,H,W], pose [B,6], K [B,3,3]
 * -> out [B,3,H,W].  flags: MCAV_WL_K_F64.  pose_inv as in the reference. */
int mcav_inverse_warp_fwd(const float* img, const float* depth, const float* pose, const void* K,
                          int B, int H, int W, int pose_inv, unsigned flags, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Its backward w.r.t. depth [B,H,W] and pose [B,6] given grad_out [B,3,H,W] (images are leaves on this path). */
int mcav_inverse_warp_bwd(const float* img, const float* depth, const float* pose, const void* K,
                          const float* grad_out, int B, int H, int W, int pose_inv, unsigned flags,
                          float* d_depth, float* d_pose, void* workspace, size_t workspace_bytes, void* stream);

/* Transform.reconstruct (transform.py:74-105): depth [B,H,W], K -> points [B,3,H,W]. */
int mcav_reconstruct(const float* depth, const void* K, int B, int H, int W, unsigned flags, float* points,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Transform.project (transform.py:114-150): points [B,3,H,W], K, Tcw [B,4,4] fp32 -> grid [B,H,W,2]. */
int mcav_project(const float* points, const void* K, const float* Tcw, int B, int H, int W, unsigned flags,
                 float* grid, void* stream);

/* transformation_from_parameters / rot_from_axisangle / get_translation_matrix (pose_geometry.py:124-199):
 * pose [B,6] = (axis-angle, translation) -> T [B,4,4] = Trans @ Rot, or its rigid inverse.  float32 as the reference; the inverse's
 * translation -R^T t is formed in float64 and rounded once (in float32 it inherits the rotation's absolute error times t). */
int mcav_pose_to_matrix(const float* pose, int B, int invert, float* T, void* stream);
/* invert_pose (pose_geometry.py:110-115): T [B,4,4] rigid -> [R^T | -R^T t]. */
int mcav_invert_pose(const float* T, int B, float* Tinv, void* stream);

/* disp_to_depth (pose_geometry.py:81-82) and its backward: n elements. */
int mcav_disp_to_depth(const float* disp, float* depth, size_t n, void* stream);
int mcav_disp_to_depth_bwd(const float* disp, const float* d_depth, float* d_disp, size_t n, void* stream);

/* The depth pyramid of the multi-scale loss: the coarse disparity maps of up to MCAV_PYR_MAX_LEVELS decoder scales -> full-resolution
 * depths, one launch forward and one backward, in place of one mcav_disp_to_depth + one mcav_resize_bilinear_fwd (and their backwards)
 * per scale and per depth pass.
 * levels: HOST array of nlevels records, copied into the kernel arguments (no device table, no copy: the call can be captured).
 *   disp:   device [B,h,w] sigmoid disparities, 1 <= h <= H, 1 <= w <= W (upsampling only, as mcav_resize_bilinear_bwd);
 *   d_disp: device [B,h,w], written by the backward (the forward ignores it).
 * B is the stacked batch: the maps of the target and the reference pass of one scale are one [2B,h,w] buffer.
 * out, d_out: device [nlevels][B][H][W].  With R = bilinear resize to H x W (F.interpolate, align_corners=False: the taps of
 * mcav_resize_bilinear_fwd with scale = h / H in float32) and D(d) = 1 / (10 d + 0.01) (mcav_disp_to_depth):
 *   default (the reference's order, losses.py:212-216):  out_l = R(D(disp_l)),  d_disp_l = D'(disp_l) * R^T(d_out_l)
 *   MCAV_PYR_RESIZE_THEN_DEPTH (monodepth2's order):     out_l = D(R(disp_l)),  d_disp_l = R^T(-10 out_l^2 * d_out_l)
 * The backward reads `out` only under MCAV_PYR_RESIZE_THEN_DEPTH (it may be NULL otherwise) and `disp` only in the default order.
 * No workspace, no host synchronisation, no atomics: every sum runs in a fixed order (along x, then along y), results are bit-identical
 * from run to run.  Returns MCAV_E_INVALID for a null pointer, nlevels outside [1, MCAV_PYR_MAX_LEVELS], a non-positive size, h > H or
 * w > W, unknown flag bits or B * H * W >= 2^31; nothing is launched then. */
#define MCAV_PYR_MAX_LEVELS 3
#define MCAV_PYR_RESIZE_THEN_DEPTH 1
typedef struct mcav_pyr_level {
    const float* disp;
    float* d_disp;
    int h, w;
} mcav_pyr_level;
int mcav_depth_pyramid_fwd(const mcav_pyr_level* levels, int nlevels, int B, int H, int W, unsigned flags, float* out, void* stream);
int mcav_depth_pyramid_bwd(const mcav_pyr_level* levels, int nlevels, int B, int H, int W, unsigned flags, const float* out,
                           const float* d_out, void* stream);

/* SSIM.standard_loss (losses.py:12-54): x, y [N,H,W] planes (N = B*C) -> clamp((1-SSIM)/2, 0, 1). */
int mcav_ssim_fwd(const float* x, const float* y, int N, int H, int W, float C1, float C2, float* out, void* stream);

/* Losses.smooth_loss for ONE scale (losses.py:242-260): depth [B,1,H,W]; loss_accum[0] += weight * term,
 * d_depth (+)= upstream[0] * weight * d term.  accumulate != 0 adds into d_depth.  The signs of a pixel's ten terms are summed exactly
 * and weighted in float64: each gradient element is rounded once. */
size_t mcav_smooth_workspace_bytes(int B, int H, int W);
int mcav_smooth_loss_fwd_bwd(const float* depth, int B, int H, int W, float weight, const float* upstream,
                             float* loss_accum, float* d_depth, int accumulate,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Edge-aware smoothness on mean-normalised disparity for ONE scale: monodepth2's get_smooth_loss(disp / (mean_disp + 1e-7), color)
 * (layers.py get_smooth_loss, trainer.py compute_losses), the smoothness term that goes with MCAV_WL_MIN_REPROJ / MCAV_WL_AUTOMASK.
 * disp: [B,1,h,w] sigmoid disparity of the target (NOT depth); img: [B,3,H,W] the target image as passed to the loss.
 * f = H / h must be an integer equal to W / w; I_s = the f x f box average of img (f = 1: img itself).  Per sample b:
 *   m_b = mean of d_b over its h*w pixels,  n = d_b / (m_b + 1e-7)
 *   wx(y,x) = exp(-(1/3) sum_c |I_s(c,y,x) - I_s(c,y,x+1)|)  (x < w-1),   wy(y,x) likewise along y  (y < h-1)
 *   E = 1/(B h (w-1)) sum_{b,y,x} |n(y,x) - n(y,x+1)| wx  +  1/(B (h-1) w) sum_{b,y,x} |n(y,x) - n(y+1,x)| wy
 * A direction without pairs (w == 1 or h == 1) contributes 0.  With R_b = the weighted sum of |d_p - d_q| of sample b (the two factors
 * included): E = sum_b R_b / (m_b + 1e-7) and dE/dd_i = dR_b/dd_i / (m_b + 1e-7) - R_b / ((m_b + 1e-7)^2 h w); |.|' at 0 is 0.
 *
 * mcav_edge_smooth_fwd: loss_accum[0] += weight * E (one float on the device; the same += contract as mcav_smooth_loss_fwd_bwd) and
 *   saved[0..B) = m_b, saved[B..2B) = R_b (2B doubles on the device, read by the backward).  Two launch-internal reductions, deterministic
 *   (float64, fixed order).  The workspace holds tickets that every launch leaves at zero: zero-fill it when it is allocated.
 * mcav_edge_smooth_bwd: d_disp (+)= upstream[0] * weight * dE/dd from the forward's saved sums; upstream: one float on the DEVICE (NULL
 *   means 1); accumulate != 0 adds into d_disp.  Needs no workspace.
 * Both return MCAV_E_INVALID for a null pointer, a non-positive size, H % h, W % w, H / h != W / w or B > 4095 (ticket capacity), and
 * the forward MCAV_E_WORKSPACE for a workspace below mcav_edge_smooth_workspace_bytes(B, h, w).  Nothing is launched then. */
size_t mcav_edge_smooth_workspace_bytes(int B, int h, int w);
int mcav_edge_smooth_fwd(const float* disp, const float* img, int B, int H, int W, int h, int w, float weight, double* saved,
                         float* loss_accum, void* workspace, size_t workspace_bytes, void* stream);
int mcav_edge_smooth_bwd(const float* disp, const float* img, int B, int H, int W, int h, int w, float weight, const double* saved,
                         const float* upstream, float* d_disp, int accumulate, void* stream);

/* Depth geometry consistency (SC-SfMLearner, Bian et al., NeurIPS 2019, compute_pairwise_loss / mean_on_mask): the two depth maps of a
 * training step must agree with each other through the pose, which keeps the scale of the prediction from drifting between frames.  The
 * definition is tests/geom_consistency_ref.py.  Two directions d, the geometries of the fused loss kernel's warps 0 and 2:
 *   d = 0: a = tgt, b = ref0, [R|t] = pose[:,0];      d = 1: a = ref0, b = tgt, [R|t] = the rigid inverse of pose[:,0].
 * For every pixel p = (x, y) of a, with D = 1 / (10 disp + 0.01) (or the inputs themselves under MCAV_WL_INPUT_DEPTH):
 *   c        = P [K^-1 [x y 1]^T D_a(p) ; 1],  P = K [R|t]
 *   (ix, iy) = the sampling position of mcav_warp_loss_fwd_bwd for that warp: c0 / (c2 + 1e-5), c1 / (c2 + 1e-5) through the
 *              normalise / un-normalise round trip, align_corners=True -- the same position and bilinear cell, bit for bit
 *   D_proj   = c2,   D_samp = the bilinear sample of D_b at (ix, iy), zero outside the image
 *   valid    = 0 <= ix <= W-1 && 0 <= iy <= H-1 && D_proj >= 1e-3   (NaN: not valid)
 *   diff     = |D_proj - D_samp| / (D_proj + D_samp)                 (|.|' at 0 is 0)
 *   n_d = number of valid pixels over the batch,  E_d = sum(valid * diff) / n_d if n_d > min_valid, else 0 with zero gradients
 *   loss_gc  = 0.5 (E_0 + E_1)
 * SC-SfMLearner clamps D_proj at 1e-3 where this drops the pixel (a clamped pixel has no gradient through D_proj either); its
 * mean_on_mask uses min_valid = 100.  The count carries no gradient.
 *
 * disp_t, disp_r0: [B,1,H,W]; poses: [B,2,6] (pose[:,1] takes no part: its gradient is 0); K: [B,3,3] fp64 (MCAV_WL_K_F64) or fp32.
 * flags: MCAV_WL_K_F64 | MCAV_WL_INPUT_DEPTH | MCAV_GC_LDS_TILE.  With MCAV_WL_INPUT_DEPTH the depths must be > 1/16 (see the scatter
 * below); depths from disparities are >= 0.0999.  MCAV_GC_LDS_TILE selects the backward's second scatter form (the forward ignores it):
 * the taps of a 32 x 32 tile of a are first added into an LDS copy of the same tile of b plus a halo of 8 and flushed with one global add
 * per non-zero texel; taps beyond the halo go straight to global memory.  Integer sums: both forms give the same bits.
 * mcav_geom_consistency_fwd: loss_accum[0] += weight * loss_gc (one float on the device, the += contract of mcav_edge_smooth_fwd).
 *   saved: 4 + 24 B doubles on the DEVICE, read by the backward: n_0, n_1, sum(valid diff)_0, _1, then the raw (unnormalised) sums
 *     d diff / dP [B][2][12].  Nothing comes back to the host.
 *   diff_out: optional [B,2,H,W] float (NULL = not written): diff of direction d in plane d, -1 where the pixel is not valid.
 *     1 - diff is SC-SfMLearner's weight mask.
 *   One memset node (the completion tickets) and one launch.  The per-workgroup partial sums (sum of diff, the valid count as an
 *   integer, the 12 dP sums) are added in float64 in a fixed order: every output is bit-identical from run to run.  diff_out, n_d
 *   (integers) and with them every gradient of a sample do not depend on where the sample sits in the batch; the float64 sums of diff
 *   over the samples are added in an order fixed by the sample INDEX, so permuting a batch of three or more samples can move saved[2..3]
 *   and the loss in the last bit (two samples: a + b = b + a).
 * mcav_geom_consistency_bwd: the same inputs and `saved`; upstream: one float on the DEVICE (NULL means 1).  With
 *   k_d = upstream * weight * 0.5 / n_d (0 when n_d <= min_valid):
 *     d_disp_t  (+)= k_0 direct_0 + k_1 scattered_1,    d_disp_r0 (+)= k_1 direct_1 + k_0 scattered_0    (times -10 D^2 for disparities)
 *     d_poses[:,0] (+)= the pose gradient of k_0 dP_0 and, through the inverse, k_1 dP_1;  d_poses[:,1] (+)= 0
 *   direct_d: d diff / d D_a through D_proj and through the sampling position; scattered_d: the adjoint of the bilinear gather, each
 *   tap's w_tap * d diff / d D_samp added to its texel of D_b.  That sum is formed in 64-bit FIXED POINT: the contribution is clamped to
 *   [-(8 - 2^-21), 8 - 2^-21], converted with llrint(g * 2^36) and added as an integer, so it does not depend on the order of arrival (no float atomics).
 *   |d diff / d D_samp| <= 1 / (2 D_samp) <= 5.005 for depths from disparities, and < 8 for depths > 1/16: the clamp never acts there;
 *   a texel receives at most one tap per pixel of a, so |sum| <= (8 - 2^-21) * 2^36 * H*W < 2^63 for H*W <= 2^24: no overflow.  accumulate != 0 adds into the three outputs.
 *   One memset node (the accumulators) and two launches (scatter, combine).
 * The workspace is scratch for the duration of one call (tickets, slab, accumulators: 24 B H W bytes and change); it needs no zero-fill
 * and carries nothing from one call to the next: a forward never depends on what an earlier call left behind.  One call at a time per
 * workspace.  No host synchronisation, allocation or copy: both calls can be captured in a hipGraph.
 * Both return MCAV_E_INVALID for a null pointer (diff_out and upstream excepted), unknown flag bits, min_valid < 0, B <= 0, B > 4095,
 * H < 2, W < 2 or H*W > 2^24, and MCAV_E_WORKSPACE for a workspace below mcav_geom_consistency_workspace_bytes(B, H, W) (which is 0 for
 * a rejected shape).  Nothing is launched then. */
#define MCAV_GC_LDS_TILE 256u
size_t mcav_geom_consistency_workspace_bytes(int B, int H, int W);
int mcav_geom_consistency_fwd(const float* disp_t, const float* disp_r0, const float* poses, const void* K, int B, int H, int W,
                              unsigned flags, int min_valid, float weight, double* saved, float* loss_accum, float* diff_out,
                              void* workspace, size_t workspace_bytes, void* stream);
int mcav_geom_consistency_bwd(const float* disp_t, const float* disp_r0, const float* poses, const void* K, int B, int H, int W,
                              unsigned flags, int min_valid, float weight, const double* saved, const float* upstream,
                              float* d_disp_t, float* d_disp_r0, float* d_poses, int accumulate,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- after the training step ------------------------------------------------------------------ */

/* Depth metrics, reference evaluate.py:6-39 (compute_errors): one pass over the ground-truth depth and the network's sigmoid
 * disparity (depth = 1 / (10 disp + 0.01), pose_geometry.py:82-83), float32 per element as the reference, float64 sums.
 * out10 (device) = { silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3, number of elements taken }.  sq_rel is the real
 * mean((gt-pred)^2 / gt); the reference returns rms under that key (evaluate.py:36).  Elements with gt <= min_gt are skipped
 * (KITTI ground truth is sparse); min_gt < 0 takes every element, as the reference does. */
size_t mcav_depth_metrics_workspace_bytes(void);
int mcav_depth_metrics(const float* gt, const float* disp, size_t n, float min_gt, float* out10, void* workspace, size_t workspace_bytes,
                       void* stream);

/* The KITTI depth evaluation protocol (monodepth2 evaluate_depth.py, monodepth evaluation_utils.py), per image, at the ground truth's own
 * resolution.  The definition is tests/eval_protocol_ref.py; for image b with true size (Hb, Wb) = sizes[b] and crop box boxes[b]:
 *   up   = disp[b] (h x w) resized to Hb x Wb, bilinear with half-pixel centres and edge clamping (F.interpolate, align_corners=False)
 *   pred = 1 / (10 up + 0.01) * scale                 float32, each operation rounded (numpy float32)
 *   mask = min_depth < gt < max_depth, inside the half-open box [y0, y1) x [x0, x1)
 *   with MCAV_EVAL_MEDIAN_SCALING: ratio = median(gt[mask]) / median(pred[mask]) (exact medians as np.median on float32), pred *= ratio
 *   pred = clip(pred, min_depth, max_depth), metrics over the mask as mcav_depth_metrics (sq_rel the squared-relative error).
 * gt: device [B,Hg,Wg] metres (0 = no return), padded: only [0, Hb) x [0, Wb) of each image is read, the padding may hold anything.
 * disp: device [B,h,w] sigmoid disparity.  sizes: device int [B,2] (Hb, Wb); boxes: device int [B,4] (y0, y1, x0, x1); both clamped in the
 * kernels (Hb to [0, Hg], the box to the true size), so no value reads out of bounds.
 * rows: device [B,11] = { silog, abs_rel, log10, rms, sq_rel, log_rms, d1, d2, d3, count, ratio } per image (ratio 1 without scaling).
 *   An image without a masked pixel gets count 0 and NaN everywhere else; a NaN prediction inside the mask makes its metrics NaN.
 * Deterministic: no float atomics, float64 sums in a fixed order; rows are bit-identical from run to run.  No host synchronisation,
 * allocation or copy: the call can be captured in a hipGraph.  10 launches with scaling, 2 without.
 * Workspace (mcav_eval_depth_workspace_bytes, each piece rounded up to 256 bytes):
 *   B * 8  +  B * 32  +  B * 32768  +  B * 8 * Hg * Wg  +  B * 88 * ceil(Hg * Wg / 2048)   bytes
 *   (counters, selection state, 2048-bin histograms, the masked gt / pred keys, the per-workgroup float64 sums).  No zero-fill needed.
 * Returns MCAV_E_INVALID for a null pointer, a non-positive size, unknown flag bits, min_depth <= 0, max_depth <= min_depth or a
 * non-finite scale, MCAV_E_WORKSPACE for a workspace below mcav_eval_depth_workspace_bytes(B, Hg, Wg); nothing is launched then. */
#define MCAV_EVAL_MEDIAN_SCALING 1
size_t mcav_eval_depth_workspace_bytes(int B, int Hg, int Wg);
int mcav_eval_depth(const float* gt, const float* disp, int B, int Hg, int Wg, int h, int w,
                    const int* sizes, const int* boxes,
                    float min_depth, float max_depth, float scale, int flags,
                    float* rows, void* workspace, size_t workspace_bytes, void* stream);
/* mcav_eval_depth with a per-image scale on the device: pred = 1 / (10 up + 0.01) * s_b, s_b = scale * scales[b] formed once in float32
 * (scales: device [B], e.g. column 0 of mcav_ground_scale's rows; NULL = mcav_eval_depth, bit for bit).  The optional median scaling and
 * everything else as there; rows[:, 10] stays the median ratio (1 without it).  A NaN s_b makes that image's metrics NaN. */
int mcav_eval_depth_scaled(const float* gt, const float* disp, int B, int Hg, int Wg, int h, int w,
                           const int* sizes, const int* boxes,
                           float min_depth, float max_depth, float scale, const float* scales, int flags,
                           float* rows, void* workspace, size_t workspace_bytes, void* stream);

/* Depth image -> pseudo-LiDAR cloud, reference pseudo-lidar/utils/PseudoLiDAR.py:69-110 (project_PL) with :39-46
 * (inverse_rigid_trans): un-project with P_rect_02, transform into the velodyne frame, keep x >= 0 and z < 1 m, keep every
 * sparsity-th survivor (0 = all), in pixel order; float64 like the reference's numpy arithmetic; 4th column 0 as in the reference.
 * depth [rows, cols] float32 on the device; T_velo_to_cam (4x4) and P_rect (3x4) are HOST pointers, row-major doubles.
 * cloud: device [capacity_points][4] doubles (rows * cols is always enough).  count_out_dev (device unsigned) receives the number of
 * valid points BEFORE sparsification: the cloud has ceil(count / max(sparsity, 1)) rows. */
size_t mcav_pseudo_lidar_workspace_bytes(int rows, int cols);
int mcav_pseudo_lidar_project(const float* depth, int rows, int cols, const double* T_velo_to_cam, const double* P_rect, int sparsity,
                              double* cloud, size_t capacity_points, unsigned* count_out_dev, void* workspace, size_t workspace_bytes,
                              void* stream);

/* A batch of network outputs -> float32 pseudo-LiDAR clouds (x, y, z, i as KITTI .bin files and sensor_msgs/PointCloud2 hold them), with
 * the resize to the calibration's resolution inside.  The definition is tests/pl_batch_ref.py.  For image b with true size
 * (Hb, Wb) = sizes[b] inside the padded (Hg, Wg), P = P[b] (3x4) and T = T[b] (4x4 velodyne -> camera), at pixel (r, c), r < Hb, c < Wb:
 *   v       = the [h, w] plane m[b] resized to (Hb, Wb) as mcav_eval_depth resizes the disparity (bilinear, half-pixel centres, edge
 *             clamping, csrc/eval_math.h bilinear_sample); m[b][r][c] itself when (h, w) == (Hb, Wb) (no taps, no 0 * inf)
 *   d       = 1 / (10 v + 0.01) * scale, float32, every operation rounded (the depth mcav_eval_depth scores); with
 *             MCAV_PLB_INPUT_DEPTH d = v * scale
 *   point   = mcav_pseudo_lidar_project's float64 sequence: x = ((c - cu) d) / fu + bx, y likewise,
 *             q_j = ((x ti[j][0] + y ti[j][1]) + d ti[j][2]) + ti[j][3], with cu, cv, fu, fv, bx, by and ti = [R' | -R' t] formed from P
 *             and T exactly as there (on the device here)
 *   keep    q0 >= 0 && q2 < max_height && d <= max_depth (a NaN fails; max_depth = +inf switches that cut off)
 *   row     = (float32(q0), float32(q1), float32(q2), i), i = 0 or the plane intensity[b] resized as m[b]
 * Dense form (elev == azim == NULL, n_beams == n_azimuth == 0): the rows of the kept pixels in (image, row-major pixel) order; with
 *   sparsity = k > 0 every k-th kept pixel of each image, the rank starting at 0 in every image (the reference's cloud[0::k] per frame).
 * Beam form: elev [n_beams + 1] holds tan(e) |tan(e)| at the beam edges, azim [n_azimuth + 1] tan(phi) at the azimuth edges, both float64,
 *   finite and strictly increasing (mcav_pl_beam_tables_check tells, on HOST copies; MCAV_E_INVALID otherwise).  A kept pixel with q0 > 0
 *   has s = q2 |q2| / (q0 q0 + q1 q1) and a = q1 / q0; its beam is the k with elev[k] <= s < elev[k+1], its azimuth bin likewise from a;
 *   outside either table, or NaN: dropped.  Per (image, beam, azimuth) cell the pixel with the smallest float32((q0 q0 + q1 q1) + q2 q2)
 *   wins, ties to the lowest pixel index; the winners' rows in (image, beam, azimuth) order.  sparsity is ignored.
 * offsets[b] .. offsets[b+1] is image b's slice of cloud (offsets[B] = the number of rows).  Rows at or beyond capacity_points are not
 * written; offsets stay exact.
 * m, intensity (or NULL): device [B, h, w] float32; sizes: device int [B, 2]; calib: device [B, 28] doubles, P (12, row-major) then T (16);
 * elev, azim: device; cloud: device [capacity_points, 4] float32, 16-byte aligned; offsets: device int [B + 1].
 * Sizes are clamped to (Hg, Wg) in the kernels, so no value reads or writes out of bounds.  Integer atomicMin only: bit-identical from run
 * to run and for any launch order.  No host synchronisation, allocation or host copy: the call can be captured.  Dense: 4 launches
 * (calibration, count, scan, scatter); beams: a memset and 5 launches (calibration, bin, count, scan, scatter).
 * Workspace (mcav_pl_batch_workspace_bytes, each piece rounded up to 256 bytes): B * 120 bytes of calibration,
 * 4 * (B * max(ceil(Hg Wg / 256), ceil(n_beams n_azimuth / 256)) + 1) of counts, 8 * B * n_beams * n_azimuth of cells.  No zero-fill needed.
 * Returns MCAV_E_INVALID for a null required pointer, a non-positive size, B * Hg * Wg, B * h * w or B * n_beams * n_azimuth >= 2^31,
 * sparsity < 0, only one of elev / azim / n_beams / n_azimuth given, a NaN scalar, a misaligned cloud or unknown flag bits, and
 * MCAV_E_WORKSPACE for a workspace below mcav_pl_batch_workspace_bytes (which is 0 for sizes it refuses); nothing is launched then. */
#define MCAV_PLB_INPUT_DEPTH 1
size_t mcav_pl_batch_workspace_bytes(int B, int Hg, int Wg, int n_beams, int n_azimuth);
int mcav_pl_beam_tables_check(const double* elev_host, int n_beams, const double* azim_host, int n_azimuth);
int mcav_pl_batch_project(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                          const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                          float scale, double max_height, double max_depth, int sparsity, int flags, float* cloud,
                          size_t capacity_points, int* offsets, void* workspace, size_t workspace_bytes, void* stream);
/* mcav_pl_batch_project with a per-image scale on the device: d = 1 / (10 v + 0.01) * s_b (or v * s_b), s_b = scale * scales[b] formed
 * once in float32 (scales: device [B]; NULL = mcav_pl_batch_project, bit for bit).  An image whose s_b is not finite or not positive keeps
 * no pixel (offsets stay exact): a fallback of NaN from mcav_ground_scale yields an empty cloud. */
int mcav_pl_batch_project_scaled(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                 const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                                 float scale, const float* scales, double max_height, double max_depth, int sparsity, int flags,
                                 float* cloud, size_t capacity_points, int* offsets, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* mcav_pl_batch_project_scaled that also records where every row came from: pixels (device int32 [capacity_points], not NULL) gets
 * pixels[o] = r * Wg + c, the pixel of its image's padded grid that became row o (the image follows from offsets), in the dense form, with
 * sparsity and in the beam form.  Rows at and beyond capacity_points are not written.  Same kernels, launches and workspace; cloud and
 * offsets are mcav_pl_batch_project_scaled's, bit for bit. */
int mcav_pl_batch_project_indexed(const float* m, int B, int h, int w, int Hg, int Wg, const int* sizes, const double* calib,
                                  const float* intensity, const double* elev, const double* azim, int n_beams, int n_azimuth,
                                  float scale, const float* scales, double max_height, double max_depth, int sparsity, int flags,
                                  float* cloud, size_t capacity_points, int* offsets, int* pixels, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* The backward of mcav_pl_batch_project_indexed: the gradient of the cloud rows -> the gradient of the plane m.  The selection (which
 * pixels became rows) is piecewise constant and has no gradient; scale, scales, intensity and the calibration get none.  The definition is
 * tests/pl_bwd_ref.py; the arithmetic is csrc/pl_bwd_math.h.  m, sizes, calib, scale, scales, flags: the forward's; pixels, offsets: what it
 * left; d_points: device [capacity_points, 4] float32, 16-byte aligned (column 3, the intensity, is ignored; rows at and beyond
 * min(offsets[B], capacity_points) are never read); d_m: device [B, h, w] float32, every element written.
 *   a) G [B, Hg, Wg] = +0.0 (a memset node), then for row o of image b at (r, c) = pixels[o]: v and s_b as the forward has them, in float64
 *      a_j = (((c - cu) / fu) ti[j][0] + ((r - cv) / fv) ti[j][1]) + ti[j][2], g_d = (g0 a_0 + g1 a_1) + g2 a_2,
 *      slope = ((-10 s_b) u) u with u = 1 / (10 v + 0.01), or s_b with MCAV_PLB_INPUT_DEPTH; G[b][r][c] = float32(g_d slope).  A pixel owns
 *      at most one row in every form.  A row whose pixel lies outside its image is skipped.
 *   b) d_m[b][y][x] = the float64 sum, rounded once, over the outputs (r, c) of image b whose taps touch (y, x), in ascending (r, c)
 *      order, of (wy(r, y) wx(c, x)) G[b][r][c] with the forward's float32 weights 1 - l and l (both added in float32 when the taps coincide
 *      at the last source); the windows by bisection over csrc/eval_math.h's bilinear_axis itself.  (h, w) == (Hb, Wb): G[b][y][x].  An image
 *      whose s_b is not finite and positive: +0.0.
 * No atomics: bit-identical from run to run.  A memset and 2 launches; no host synchronisation, allocation or copy: the call can be
 * captured.  Workspace (mcav_pl_batch_project_bwd_workspace_bytes, 0 for sizes that are refused): the plane G, 4 B Hg Wg bytes rounded up
 * to 256, 4-byte aligned; no zero-fill needed.
 * Returns MCAV_E_INVALID for a null pointer (scales may be NULL), a non-positive size, B * Hg * Wg or B * h * w >= 2^31, a NaN scale, a
 * misaligned d_points or workspace or unknown flag bits, MCAV_E_WORKSPACE for a short workspace; nothing is launched then. */
size_t mcav_pl_batch_project_bwd_workspace_bytes(int B, int Hg, int Wg);
int mcav_pl_batch_project_bwd(const float* d_points, size_t capacity_points, const int* pixels, const int* offsets, const float* m, int B,
                              int h, int w, int Hg, int Wg, const int* sizes, const double* calib, float scale, const float* scales,
                              int flags, float* d_m, void* workspace, size_t workspace_bytes, void* stream);

/* Metric scale of a monocular prediction from the ground plane (DNet's dense geometrical constraint, Xue et al., IROS 2020): per image, a
 * surface normal per pixel from the back-projected depth, the pixels whose normal points along the camera's "down" axis, and
 * scale = camera_height / median(height of those pixels above the plane through the camera centre).  No ground truth is read.
 * The definition is tests/ground_scale_ref.py; per-pixel math: csrc/ground_math.h.  For image b of m [B, h, w] with true size
 * (Hb, Wb) = sizes[b] and P = P[b] (fu = P00, fv = P11, cu = P02, cv = P12), float32 with every operation rounded on its own:
 *   rays    xn[c] = float32((((c + 0.5) Wb) / w - 0.5 - cu) / fu), the inner arithmetic in float64 in that order; yn[r] alike from Hb, h,
 *           cv, fv: the native pixel a network pixel centre maps to under mcav_eval_depth's half-pixel resize
 *   depth   d = 1 / (10 v + 0.01); with MCAV_GS_INPUT_DEPTH d = v.           point  Pt = (xn[c] d, yn[r] d, d)
 *   normal  for an interior pixel (1 <= r <= h-2, 1 <= c <= w-2) inside the box: e_k = Pt(neighbour k) - Pt(centre) for R, D, L, U, DR, DL,
 *           UL, UR; the cross products (R,D) (D,L) (L,U) (U,R) (DR,DL) (DL,UL) (UL,UR) (UR,DR), cx = a.y b.z - a.z b.y and so on,
 *           len = sqrt((cx cx + cy cy) + cz cz), u = c / len; acc = the eight u summed in that order from +0; L = |acc|, n = acc / L
 *   height  hgt = (n.x X + n.y Y) + n.z Z of the centre
 *   ground  every len and L finite and > 0, n.y >= cos_max, hgt finite and > 0 (a NaN fails every test)
 *   rows[b] = { scale, med, count, status }: count ground pixels, med their exact median as np.median on float32 (NaN without any),
 *           count >= min_ground: scale = camera_height / med, status 1; otherwise scale = fallback, status 0.
 * m: device [B, h, w]; sizes: device int [B, 2]; calib: device [B, 28] doubles as mcav_pl_batch_project takes them (only P is read);
 * boxes: device int [B, 4] (y0, y1, x0, x1) in network pixels, half-open, clamped in the kernel, or NULL (the whole interior);
 * rows: device [B, 4]; mask_out: device [B, h, w] bytes, 1 on ground pixels, or NULL.
 * Two launches: a pixel pass (one workgroup per 8 x 32 tile of the image's interior, the tile's points and a one-pixel halo in LDS) that
 * leaves a key per interior pixel -- the bits of hgt, which order positive floats, or 0xFFFFFFFF -- and one workgroup per image that
 * selects both median ranks exactly from those keys over 11 + 11 + 10 bits.  LDS integer atomics only; rows and mask are bit-identical
 * from run to run.  No host synchronisation, allocation or copy: the call can be captured.
 * Workspace (mcav_ground_scale_workspace_bytes): 4 * B * (h - 2) * (w - 2) bytes, rounded up to 256, 4-byte aligned; no zero-fill.
 * Returns MCAV_E_INVALID for a null required pointer, h < 3, w < 3, B <= 0, B * h * w >= 2^31, a camera_height that is not finite and
 * positive, cos_max outside (0, 1], min_ground < 1, unknown flag bits or a workspace address that is no multiple of 4, MCAV_E_WORKSPACE
 * for a short workspace; nothing is launched then. */
#define MCAV_GS_INPUT_DEPTH 1
size_t mcav_ground_scale_workspace_bytes(int B, int h, int w);
int mcav_ground_scale(const float* m, int B, int h, int w, const int* sizes, const double* calib, const int* boxes, float camera_height,
                      float cos_max, int min_ground, float fallback, int flags, float* rows, unsigned char* mask_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* Cloud batch -> pillars, the input of a LiDAR 3-D detector (PointPillars / SECOND / OpenPCDet: voxels [P, N, C], coords [P, 4],
 * num_points [P]).  The definition is tests/pillar_ref.py; the arithmetic is csrc/pillar_math.h.
 *   input    points [n_max, 4] float32 (x, y, z, i) and offsets int32 [B + 1] (offsets[0] = 0, ascending) on the device, as
 *            mcav_pl_batch_project leaves them: image b owns rows offsets[b] .. offsets[b + 1]; n = min(offsets[B], n_max) and rows at and
 *            beyond n are never read.  The host does not know n: launches are sized by n_max.
 *   grid     nx x ny cells of vx x vy from (x0, y0), one cell in z: [z0, z1)
 *   cell     float32, every operation rounded on its own: fx = floorf((x - x0) / vx) (IEEE division), fy likewise; the point is kept iff
 *            0 <= fx < nx, 0 <= fy < ny and z0 <= z < z1, compared as floats and converted to int only then: a NaN or an infinite
 *            coordinate drops the point, -0.0 is 0.  Cell = (b, iy, ix).
 *   pillars  the non-empty cells in ascending (b, iy, ix) order; pillar_offsets int32 [B + 1]: image b owns pillars
 *            pillar_offsets[b] .. pillar_offsets[b + 1], exact whatever the capacity; rows at and beyond capacity are not written.
 *   slots    the points of the cell with the min(count, max_points) smallest row indices, in ascending index order (second.pytorch's
 *            "first N in cloud order"); num_points = min(count, max_points); the slots behind them are +0.0 in every column.
 *   coords   (b, 0, iy, ix): OpenPCDet's (batch, z, y, x)
 *   columns  C = 4: x, y, z, i, copied bit for bit.  MCAV_PILLAR_DECORATE: C = 9; columns 4..6 = x - mx, y - my, z - mz with m the float64
 *            sum over the kept slots in slot order, divided by num_points in float64 and rounded once to float32; columns 7..8 =
 *            x - ((float)ix * vx + (vx * 0.5f + x0)) and the same in y, every product and sum rounded on its own.
 * voxels: device [capacity, max_points, C] float32; coords: device [capacity, 4] int32; num_points: device [capacity] int32.
 * Integer atomics only, and no output depends on the order in which they land: two runs give the same bytes.  No host synchronisation,
 * allocation or copy (one hipMemsetAsync of the cell counters): the call can be captured.  6 launches.
 * Workspace (mcav_pillarize_workspace_bytes, 0 for sizes that are refused; scratch of one call, no zero-fill, each piece rounded up to 256
 * bytes): 4 (B ny nx + 1) + 8 ceil(B ny nx / 1024) + 12 n_max + 4 min(n_max, B ny nx) bytes.
 * Returns MCAV_E_INVALID for a null pointer, B <= 0, B > 65535, n_max < 0, n_max >= 2^31, B * ny * nx >= 2^31, nx or ny < 1, max_points
 * outside [1, 64], capacity < 0, a vx or vy that is not finite and positive, a non-finite x0 or y0, z1 <= z0 (a NaN included), unknown flag
 * bits, a points, coords or workspace address that is no multiple of 16, or a voxels address that is no multiple of 16 when
 * max_points * C is a multiple of 4 (the row blocks then go out in 16-byte stores; of 4 otherwise); MCAV_E_WORKSPACE for a short
 * workspace; nothing is launched then. */
#define MCAV_PILLAR_DECORATE 1
size_t mcav_pillarize_workspace_bytes(int B, long long n_max, int ny, int nx);
int mcav_pillarize(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1, float vx,
                   float vy, int nx, int ny, int max_points, int flags, float* voxels, int* coords, int* num_points, long long capacity,
                   int* pillar_offsets, void* workspace, size_t workspace_bytes, void* stream);
/* mcav_pillarize that also records which cloud row every slot holds: slot_points (device int32 [capacity, max_points], not NULL) gets the
 * row's index in `points`, -1 in the zero-padded slots.  Rows at and beyond min(pillar_offsets[B], capacity) are not written.  Same
 * kernels, launches and workspace; every other output is mcav_pillarize's, bit for bit. */
int mcav_pillarize_indexed(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float z1, float vx,
                           float vy, int nx, int ny, int max_points, int flags, float* voxels, int* coords, int* num_points,
                           long long capacity, int* pillar_offsets, int* slot_points, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The backward of mcav_pillarize_indexed: the gradient of the voxels -> the gradient of the cloud rows.  Which row lands in which slot is
 * piecewise constant and has no gradient.  The definition is tests/pl_bwd_ref.py; the arithmetic is csrc/pl_bwd_math.h.
 * d_voxels: device [capacity, max_points, C] float32 (C = 9 with MCAV_PILLAR_DECORATE, else 4; rows at and beyond
 * P = min(pillar_offsets[B], capacity) are never read); slot_points, num_points, pillar_offsets: what the forward left;
 * d_points: device [n_max, 4] float32, 16-byte aligned, every row written.  Slot k < count = num_points[p] of pillar p holding row i:
 *   C = 4   d_points[i][c] = g[k][c]
 *   C = 9   d_points[i][0] = float32((((double)g[k][0] + g[k][4]) + g[k][7]) - S4 / count), S4 = the float64 sum of g[j][4] over
 *           j = 0 .. count - 1 in slot order from +0 (the mean's derivative; the cell's centre is a constant); y from columns 1, 5, 8 and
 *           S5; z from columns 2, 6 and S6 (no centre column); column 3 passes through.
 * A row is in at most one slot: no atomics, the same bytes from run to run.  A row that no slot holds (beyond the first max_points of its
 * cell, outside the grid, in a pillar beyond the capacity) is +0.0.  A memset and one launch, one wavefront per pillar; no workspace, no
 * host synchronisation: the call can be captured.
 * Returns MCAV_E_INVALID for a null pointer, B <= 0, B > 65535, n_max < 0, n_max >= 2^31, capacity < 0, max_points outside [1, 64],
 * unknown flag bits, a d_points address that is no multiple of 16 or a d_voxels address that is no multiple of 4; nothing is launched
 * then. */
int mcav_pillarize_bwd(const float* d_voxels, const int* slot_points, const int* num_points, const int* pillar_offsets, int B,
                       long long capacity, int max_points, int flags, float* d_points, long long n_max, void* stream);

/* Cloud batch -> soft-occupancy canvas, the input of a detector that reads a dense voxel grid (PIXOR): End-to-End Pseudo-LiDAR's
 * differentiable quantisation.  The definition is tests/quant_ref.py; the arithmetic is csrc/quant_math.h.
 *   input    points, offsets, B, n_max: as mcav_pillarize takes them; n = min(offsets[B], n_max), rows at and beyond n are never read.
 *   grid     nx x ny x nz cells of vx x vy x vz from (x0, y0, z0)
 *   cell     mcav_pillarize's rule on all three axes: fz = floorf((z - z0) / vz) as fx and fy, the point is kept iff 0 <= fx < nx,
 *            0 <= fy < ny and 0 <= fz < nz, compared as floats (a NaN or an infinity drops the point); n(m') = the kept points of an
 *            image in cell m'.
 *   centre   cx = (float)ix * vx + (vx * 0.5f + x0), likewise cy, cz: float32, every operation rounded on its own
 *   term     for a kept point p of cell m' and every cell m of the 3 x 3 x 3 block around m' inside the grid: dx = x - cx(m), dy, dz;
 *            d2 = dx * dx, d2 = fmaf(dy, dy, d2), d2 = fmaf(dz, dz, d2); t = -(d2 / sigma2) (IEEE division); e = quant_exp(t), the
 *            float32 exponential of csrc/quant_math.h (at most 0.9375 ulp from exp(t); +0 for t < -87)
 *   sum      q = llrint((double)e * 2^40 / (double)(n(m') * (m == m' ? 1 : 26))); S(m) = the 64-bit integer sum of q over every term that
 *            lands on m; canvas[b, iz, iy, ix] = (float)((double)S(m) * 2^-40): E2E-PL's T(m) = T(m, m) + 1/26 sum over the neighbours m'
 *            of T(m, m'), T(m, m') the mean of e over the points of m'.  |N_m| is 26 everywhere: a neighbour outside the grid is empty.
 *   canvas   device [B, nz, ny, nx] float32; one call writes every element: no zero-fill by the caller.
 *   point_count  device int32 [n_max] or NULL: n(m') of every kept row below n, 0 for a dropped one; rows at and beyond n are not written.
 * Integer atomics only and integer sums: no output depends on the order in which they land, any number of points may share a cell, two
 * runs give the same bytes.  No host synchronisation, allocation or copy (one hipMemsetAsync of the column counters): the call can be
 * captured.  7 launches (5 when n_max = 0): a counting sort of the rows by (b, iy, ix), then one workgroup per 4 x 64 columns of an image
 * for the cell counts and for the canvas, whose tile of sums lives in LDS (512 nz bytes of it per column).
 * Workspace (mcav_cloud_occupancy_workspace_bytes, 0 for sizes that are refused; scratch of one call, no zero-fill, each piece rounded up
 * to 256 bytes): 4 (B ny nx + 1) + 4 ceil(B ny nx / 1024) + 16 n_max bytes.
 * Returns MCAV_E_INVALID for a null points, offsets, canvas or workspace, B <= 0, B > 65535, n_max < 0, n_max >= 2^31, nx or ny < 1, nz
 * outside [1, 64], B * nz * ny * nx >= 2^31, a vx, vy, vz or sigma2 that is not finite and positive, a non-finite x0, y0 or z0, a
 * points, canvas or workspace address that is no multiple of 16, or an offsets or point_count address that is no multiple of 4;
 * MCAV_E_WORKSPACE for a short workspace; nothing is launched then. */
size_t mcav_cloud_occupancy_workspace_bytes(int B, long long n_max, int nz, int ny, int nx);
int mcav_cloud_occupancy(const float* points, const int* offsets, int B, long long n_max, float x0, float y0, float z0, float vx, float vy,
                         float vz, int nx, int ny, int nz, float sigma2, float* canvas, int* point_count /* may be null */,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The backward of mcav_cloud_occupancy: the gradient of the canvas -> the gradient of the cloud rows.  The counts and the fixed-point
 * rounding are piecewise constant: the derivative is that of the unrounded expression.  points, offsets, the grid and sigma2 are the
 * forward's, point_count what it recorded; d_canvas: device [B, nz, ny, nx] float32; d_points: device [n_max, 4] float32, every row
 * written.  A kept row i below n with count c = point_count[i], its cell recomputed from the point as in the forward:
 *   d_points[i][0] = (float) sum over the cells m of the 3 x 3 x 3 block inside the grid, in ascending (dz, dy, dx) order from +0.0, of
 *                    (((double)d_canvas[m] * (w / (double)c)) * (double)e) * ((-2.0 * (double)dx) / (double)sigma2)
 *   with w = 1.0 for the point's own cell and 1.0 / 26.0 for a neighbour, e and dx the forward's float32 values, every operation float64
 *   and rounded on its own; columns 1 and 2 likewise with dy and dz.  Column 3, every dropped row and every row at and beyond n: +0.0.
 * A row has one destination: no atomics, the same bytes from run to run.  1 launch, one thread per row, no workspace, no host
 * synchronisation: the call can be captured.
 * Returns MCAV_E_INVALID for a null pointer, what the forward refuses of B, n_max, the grid and sigma2, a points or d_points address that
 * is no multiple of 16 or an offsets, point_count or d_canvas address that is no multiple of 4; nothing is launched then. */
int mcav_cloud_occupancy_bwd(const float* points, const int* offsets, const int* point_count, const float* d_canvas, int B, long long n_max,
                             float x0, float y0, float z0, float vx, float vy, float vz, int nx, int ny, int nz, float sigma2,
                             float* d_points, void* stream);

/* Pillars -> pillar features -> bird's-eye-view pseudo-image, the first layers of a LiDAR 3-D detector (PointPillars / SECOND / OpenPCDet:
 * PillarVFE's Linear + BatchNorm1d + ReLU + max over the pillar's points with the BatchNorm folded into the layer, then
 * PointPillarScatter), in one launch.  The definition is tests/pfn_ref.py; the arithmetic is csrc/pfn_math.h.
 *   input    voxels [capacity, max_points, columns] float32, coords [capacity, 4] int32 = (b, 0, iy, ix), num_points [capacity] int32 and
 *            pillar_offsets int32 [B + 1] on the device, as mcav_pillarize leaves them: rows in ascending (b, iy, ix) order, image b owns
 *            rows pillar_offsets[b] .. pillar_offsets[b + 1]; P = min(pillar_offsets[B], capacity) and rows at and beyond P are never read.
 *   layer    weight [c_out, columns], bias [c_out], bias_pad [c_out] float32 on the device; c_out a multiple of 32 in 32..128
 *   pre      for pillar p, slot k, channel o: acc = bias[o], then acc = fmaf(voxels[p, k, c], weight[o, c], acc) for c = 0 .. columns - 1
 *            in ascending order: float32, one rounding per column
 *   act      acc > 0 ? acc : (acc != acc ? acc : +0.0f): a NaN stays a NaN; -0.0, negative values and -inf give +0.0
 *   feat     feat[p, o] = the NaN-propagating maximum (torch.max, not fmaxf) of act over the slots k < n, n = num_points[p] clamped to
 *            [0, max_points]; if n < max_points, act(bias_pad[o]) joins the maximum: what second.pytorch and OpenPCDet compute, which put
 *            the zero-masked padding rows through the layer, when bias_pad = bias; any bias_pad <= 0 ignores the padding.  Which NaN comes
 *            out is not defined.
 *   canvas   device [B, c_out, ny, nx] float32 (MCAV_PFN_NHWC: [B, ny, nx, c_out]): canvas[b, o, iy, ix] = feat[p, o] for the row p with
 *            coords[p] = (b, *, iy, ix), +0.0 in every other element.  One call writes every element: no zero-fill by the caller.
 *   features device [capacity, c_out] float32 or NULL: feat in the rows below P; rows at and beyond P are not written.
 * A row whose (b, iy, ix) lies outside the canvas is skipped (with a canvas its features row is not written either); rows that are not in
 * ascending order give an unspecified canvas; neither reads or writes outside the buffers.  canvas may be NULL when features is not: the
 * features alone, for every row below P whatever its coords hold (nx and ny are still checked).
 * No atomics, no workspace, no host synchronisation, allocation or copy: the call can be captured, and two runs give the same bytes.
 * 1 launch.  A canvas whose address is a multiple of 16 (and, for [B, c_out, ny, nx], nx a multiple of 4) goes out in 16-byte stores.
 * Returns MCAV_E_INVALID for a null voxels, coords, num_points, pillar_offsets, weight, bias or bias_pad, canvas and features both null,
 * an address that is no multiple of 4, B <= 0, B > 65535, capacity < 0, nx or ny < 1, B * ny * nx >= 2^31, max_points outside [1, 64],
 * columns outside {4, 9}, c_out outside {32, 64, 96, 128} or unknown flag bits; nothing is launched then. */
#define MCAV_PFN_NHWC 1      /* canvas [B, ny, nx, C_out] instead of [B, C_out, ny, nx] */
int mcav_pillar_pseudo_image(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets,
                             int B, long long capacity, int max_points, int columns, int nx, int ny,
                             const float* weight, const float* bias, const float* bias_pad, int c_out, int flags,
                             float* canvas, float* features /* may be null */, void* stream);

/* The backward of mcav_pillar_pseudo_image: from the gradient of the canvas (and / or of the feature rows) to the gradients of the layer
 * and, when asked for, of the voxels.  The definition is tests/pfn_bwd_ref.py; the arithmetic is csrc/pfn_bwd_math.h.  The inputs are the
 * forward's, with the same P = min(pillar_offsets[B], capacity); nothing of the forward is kept, the layer is recomputed.
 *   d_canvas   device, in the forward's layout (MCAV_PFN_NHWC selects it as there), or NULL
 *   d_features device [capacity, c_out] float32, or NULL; at least one of the two is given
 *   g          g[p, o] for p < P: d_canvas[b, o, iy, ix] when the row's (b, iy, ix) lies inside the canvas, +0.0 otherwise or without a
 *              d_canvas; with d_features, d_features[p, o] is added to it in float32.  Elements of d_canvas at cells without a pillar are
 *              never read.
 *   winner     pre, act and m = feat[p, o] are the forward's, bit for bit.  Gradient flows iff m > 0 (not for a NaN; relu'(0) = 0).  It goes
 *              to the lowest slot k < n with act(pre[p, k, o]) == m; if no used slot attains m, the padding term act(bias_pad[o]) won
 *              (only possible with n < max_points); a tie between a slot and the padding goes to the slot.
 *   d_weight   [c_out, columns]: d_weight[o, c] = sum over the (p, o) won by a slot of g[p, o] * voxels[p, k, c]
 *   d_bias     [c_out]: the sum of g[p, o] over the same set;  d_bias_pad [c_out]: the sum over the (p, o) won by the padding.
 *              Every term of the three is formed in float64 (the product of two float32 is exact there), they are added in float64 in
 *              a fixed order and rounded once to float32.
 *   d_voxels   device [capacity, max_points, columns] float32, or NULL: for p < P, acc = +0.0f, then for o ascending
 *              acc = fmaf(g[p, o], weight[o, c], acc) whenever the gradient of (p, o) goes to slot k.  Every element of every row up to
 *              capacity is written: +0.0 in slots without a winner and in rows at and beyond P.
 * No float atomics, two runs give the same bytes; no host synchronisation, allocation or copy: the call can be captured.  Unsorted rows
 * and rows outside the canvas never read or write outside the buffers.  2 launches.
 * Workspace: mcav_pillar_pseudo_image_bwd_workspace_bytes (0 for sizes that are refused): 8 c_out (columns + 2) min(ceil(capacity / 64),
 * 1024) bytes rounded up to 256, scratch of one call, no zero-fill.
 * Returns MCAV_E_INVALID for what the forward refuses, d_canvas and d_features both null, a null d_weight, d_bias, d_bias_pad or
 * workspace, an address that is no multiple of 4 (the workspace: of 8); MCAV_E_WORKSPACE for a short workspace; nothing is launched
 * then. */
size_t mcav_pillar_pseudo_image_bwd_workspace_bytes(long long capacity, int columns, int c_out);
int mcav_pillar_pseudo_image_bwd(const float* voxels, const int* coords, const int* num_points, const int* pillar_offsets,
                                 int B, long long capacity, int max_points, int columns, int nx, int ny,
                                 const float* weight, const float* bias, const float* bias_pad, int c_out, int flags,
                                 const float* d_canvas /* may be null */, const float* d_features /* may be null */,
                                 float* d_weight, float* d_bias, float* d_bias_pad, float* d_voxels /* may be null */,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* The moments of a PillarBatch's used voxel slots: what training-mode BatchNorm statistics behind a linear layer without bias follow from.
 * With y = W x over all P max_points rows of the padded [P, max_points, columns] tensor (a zero-padded slot gives y = 0, as
 * second.pytorch's masked rows do), mean_o = w_o . s / rows and E[y_o^2] = w_o^T M w_o / rows.  The definition is tests/pfn_stats_ref.py;
 * the arithmetic is csrc/pfn_stats_math.h.  voxels, num_points, pillar_offsets, B, capacity, max_points, columns: as
 * mcav_pillar_pseudo_image takes them, with the same P = min(pillar_offsets[B], capacity) and n = num_points[p] clamped to
 * [0, max_points]; unused slots and rows at and beyond P are never read.
 *   moments  device float64 [2 + columns + columns^2]:
 *            [0]  rows = P max_points;  [1]  used = the sum of n over p < P
 *            [2 .. 2 + columns)  s[c] = the sum of voxels[p, k, c] over the used slots (p < P, k < n)
 *            the rest  M[c][c'] = the sum of voxels[p, k, c] voxels[p, k, c'], row-major, both halves holding the same bits
 *            A term is the float64 product of two float32 values (exact); the sums are float64 in a fixed order.  Non-finite used
 *            values propagate.
 * No atomics, two runs give the same bytes; no host synchronisation, allocation or copy: the call can be captured.  2 launches.
 * Workspace: mcav_pillar_moments_workspace_bytes (0 for sizes that are refused): 8 (1 + columns + columns (columns + 1) / 2)
 * min(ceil(capacity / 256), 512) bytes rounded up to 256, scratch of one call, no zero-fill.
 * Returns MCAV_E_INVALID for a null voxels, num_points, pillar_offsets, moments or workspace, an address that is no multiple of 4 (moments
 * and the workspace: of 8), B <= 0, B > 65535, capacity < 0, max_points outside [1, 64] or columns outside {4, 9}; MCAV_E_WORKSPACE for a
 * short workspace; nothing is launched then. */
size_t mcav_pillar_moments_workspace_bytes(long long capacity, int max_points, int columns);
int mcav_pillar_moments(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity,
                        int max_points, int columns, double* moments, void* workspace, size_t workspace_bytes, void* stream);

/* The adjoint of mcav_pillar_moments: from g [columns] float64, the gradient with respect to s, and H [columns, columns] float64, the
 * gradient with respect to M (any matrix), to the gradient of the voxels.  rows and used have no gradient.
 *   d_voxels device [capacity, max_points, columns] float32, every element written: for a used slot acc = g[c], then for c' ascending
 *            acc = fma(H[c][c'] + H[c'][c], (double)voxels[p, k, c'], acc) in float64, stored as (float)acc: one rounding; +0.0 in unused
 *            slots and in rows at and beyond P.
 * Two runs give the same bytes; no host synchronisation, allocation or copy: the call can be captured.  1 launch.
 * Returns MCAV_E_INVALID for what mcav_pillar_moments refuses of the shared arguments, a null g, H or d_voxels, or a g or H whose address
 * is no multiple of 8; nothing is launched then. */
int mcav_pillar_moments_bwd(const float* voxels, const int* num_points, const int* pillar_offsets, int B, long long capacity,
                            int max_points, int columns, const double* g, const double* H, float* d_voxels, void* stream);

/* Graph-based depth correction from sparse LiDAR (GDC): You et al., "Pseudo-LiDAR++: Accurate Depth for 3D Object Detection in Autonomous
 * Driving", ICLR 2020, section 4; the reference's notes pseudo-lidar/PL_development/research/pseudo_lidar++.md: "create a KNN graph; use
 * sparse LiDAR point clouds to bias and correct depth".  A predicted depth map has the right local shape and a smooth error; a few exact
 * LiDAR depths are propagated over it while the local shape is kept.  The definition is tests/gdc_ref.py; the per-pixel arithmetic is
 * csrc/gdc_math.h.  depth, sparse: device [B, H, W] float32 on one grid (sparse is 0 where there is no return); K: device [B, 4] float32
 * = (fx, fy, cx, cy) of that grid.
 *
 * mcav_gdc_graph -- the windowed KNN graph and its locally-linear-embedding weights:
 *   valid    min_depth < depth <= max_depth, compared as floats (NaN and +-inf drop out); known: valid and sparse in the same range
 *   point    X = ((u - cx) / fx * z, (v - cy) / fy * z, z), float32, every quotient and product rounded on its own; positions come from
 *            the PREDICTED depth for known pixels too (Pseudo-LiDAR++)
 *   graph    the candidates of pixel i are the valid j != i of the (2 radius + 1)^2 window around it, clipped to the image, whose squared
 *            distance ((dx dx + dy dy) + dz dz) is below +inf; its neighbours are the min(k, #candidates) nearest, ties to the lower
 *            pixel index, stored in ascending (distance, index) order.  A window that covers the image gives exact KNN.
 *   weights  sklearn.manifold.barycenter_weights on the scalar depths: d_j = z_j - z_i, C = d d^T + lam I, lam = reg |d|^2 (reg where
 *            |d|^2 = 0), w = C^-1 1 / sum(C^-1 1), through Sherman-Morrison: w_j ~ 1 - d_j s / (lam + q), s = sum d_j, q = sum d_j^2 in
 *            neighbour order
 *   nbr      device int32 [B, H, W, k]: v * W + u of the neighbour, -1 in unused slots; weights: device float32 [B, H, W, k], +0.0 in
 *            unused slots; flags: device uint8 [B, H, W]: bit 0 = in the graph (valid, with a candidate), bit 1 = known.
 *   One launch; every element of nbr, weights and flags is written.
 *
 * mcav_gdc_solve -- with M = I - W over the graph pixels, L the known graph pixels and U the others: z'_L = sparse_L, z'_U minimises
 * |M z'|^2.  Conjugate gradient on the normal equations from z'_U = depth_U: r = -(M^T M z')_U, p = r, rs = |r|^2, then per iteration
 *   q = M p, alpha = rs / |q|^2, z'_U += alpha p, r -= alpha (M^T q)_U, rs' = |r|^2, beta = rs' / rs, p = r + beta p.
 * Vectors and weights are float32; inner products are float64 (per-workgroup sums added in a fixed order by the image's last workgroup);
 * (M v)_i sums in neighbour order, (M^T q)_j in ascending source order (a CSR built by scanning j's window: no atomics, no sort).  An
 * image is done once rs <= tol^2 rs0, rs is not positive or |q|^2 is not positive; at most `iters` iterations; the workgroups of a
 * finished image exit on its flag.
 *   out      device [B, H, W] float32: z' on graph pixels (a known graph pixel holds its sparse value bit for bit), the bits of depth
 *            elsewhere; an image with fewer than min_known known graph pixels is passed through unchanged
 *   info     device [B, 4] float32: graph pixels, known graph pixels, iterations run, rs / rs0 (1 for a passed-through image, 0 where
 *            rs0 is not positive)
 * nbr entries outside [0, H W) are skipped, so no graph makes the call read out of bounds.  7 + 3 iters launches and one
 * hipMemsetAsync of the call's counters and tickets; no host synchronisation, allocation or float atomics: the call can be captured,
 * and two runs give the same bytes.
 * Workspace (mcav_gdc_workspace_bytes, 0 for sizes that are refused; scratch of one call, shared by both entries; each piece rounded up
 * to 256 bytes): (8 k + 12) B H W + 4 B G 256 + 12 B G + 12 B ceil(G / 16) + 44 B bytes with G = ceil(H W / 256).
 * Both return MCAV_E_INVALID for a null pointer, B <= 0, B > 65535, H or W <= 0, H W > 2^24, k outside [1, 16], radius outside [1, 7],
 * k B G 256 >= 2^31; mcav_gdc_graph also for a reg that is not positive and finite, min_depth < 0 or max_depth <= min_depth (a NaN
 * included), more than 65535 tile rows; mcav_gdc_solve also for iters < 0, a tol that is negative or NaN, out == depth or sparse, a
 * workspace address that is no multiple of 16; MCAV_E_WORKSPACE for a short workspace; nothing is launched then. */
size_t mcav_gdc_workspace_bytes(int B, int H, int W, int k, int radius);
int mcav_gdc_graph(const float* depth, const float* sparse, const float* K, int B, int H, int W, int k, int radius, float reg, float min_depth,
                   float max_depth, int* nbr, float* weights, unsigned char* flags, void* workspace, size_t workspace_bytes, void* stream);
int mcav_gdc_solve(const float* depth, const float* sparse, const int* nbr, const float* weights, const unsigned char* flags, int B, int H,
                   int W, int k, int radius, int min_known, int iters, float tol, float* out, float* info, void* workspace,
                   size_t workspace_bytes, void* stream);

/* KITTI Eigen ground truth from raw Velodyne scans (monodepth2 kitti_utils.generate_depth_map), the forward direction of the projection
 * above: scan -> sparse depth map, per image of a batch.  The definition is tests/velo_ref.py; for image b with points p = (x, y, z, r)
 * (float32, as stored in the .bin file; r is never read), P = P[b] (3x4 velodyne -> image, float64) and true size (Hb, Wb) = sizes[b]:
 *   keep          x >= 0 in float32 (NaN fails, -0.0 passes)
 *   project       q_k = ((P[k,0] x + P[k,1] y) + P[k,2] z) + P[k,3], k = 0, 1, 2: float64, x, y, z widened exactly, every operation
 *                 rounded on its own (no FMA), in this order
 *   pixel         u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1: IEEE float64 division, round half to even (np.round; not C's round())
 *   land          u >= 0 && v >= 0 && u < Wb && v < Hb, compared in float64 (NaN and +-inf fail), converted to int only then
 *   depth         d = q2; with MCAV_VELO_DEPTH_FROM_X (monodepth2's vel_depth=True) d = (double)x
 *   out[b][v][u'] = float32 of the minimum d over the points that land on that pixel, u' = Wb - 1 - u when flip[b] != 0, else u;
 *                 +0.0 where no point lands and where that minimum has its float32 sign bit set (monodepth2's depth[depth < 0] = 0:
 *                 points with 0 <= x < ~0.27 m lie behind the camera and can land with q2 < 0); +inf (a depth above FLT_MAX) is kept.
 *   [Hb, Hg) x [0, Wg) and [0, Hb) x [Wb, Wg) are 0: out is the zero-padded [B, Hg, Wg] map that mcav_eval_depth takes with sizes.
 * Differences from monodepth2: its duplicate resolution (sub2ind = row * (W - 1) + col - 1) aliases pixel (r, W-1) with (r+1, 0), so on
 * columns 0 and W-1 its result depends on the order of the points; this is the plain per-pixel minimum everywhere.  The Garg and Eigen crops
 * exclude both columns.  monodepth2 forms P p with np.dot (a BLAS order), which can differ from the fixed order above by one float64 ulp.
 * points: device [N,4] float32, the scans concatenated as read; offsets: device [B+1], image b owns points [offsets[b], offsets[b+1]);
 * P: device [B,12] row-major; sizes: device int [B,2] (Hb, Wb); flip: device [B] or NULL (no flips); out: device [B,Hg,Wg] float32.
 * max_points bounds the grid: each image's range is clamped to max_points points and sizes to [0, Hg] x [0, Wg] in the kernel, so no value
 * reads or writes out of bounds (offsets must lie inside points).  out holds the minima as order-preserving keys while the call runs (integer
 * atomicMin, no workspace): the map is bit-identical from run to run and for any order of the points within a scan.  No host
 * synchronisation, allocation or copy: the call can be captured in a hipGraph.  3 launches (init, scatter, finalize).
 * Returns MCAV_E_INVALID for a null required pointer, B, Hg or Wg <= 0, B > 65535, B * Hg * Wg * 4 >= 2^62, max_points < 0 or unknown flag
 * bits; nothing is launched then. */
#define MCAV_VELO_DEPTH_FROM_X 1
int mcav_velo_depth_map(const float* points, const long long* offsets, const double* P, const int* sizes, const unsigned char* flip,
                        int B, int Hg, int Wg, long long max_points, int flags, float* out, void* stream);

/* ---- before the training step ------------------------------------------------------------------------ */

/* The reference's image transform chain (dataloaders.py:32-49 load_img, trainer.py:97-103): decoded uint8 RGB -> /255 -> ToTensor ->
 * ToPILImage -> Resize((h, w)) [Pillow bilinear, antialiased, 8-bit fixed point, horizontal then vertical] -> ToTensor -> Normalize,
 * for a batch of equally sized images, bit-exact against Pillow's resize.
 * mcav_resample_coeffs (HOST): Pillow's coefficient tables for one axis; call it with kk = NULL to get the capacity (out_size * ksize)
 * and *ksize_out, then again with host arrays bounds[out_size * 2], kk[capacity]; copy both to the device for mcav_image_preprocess.
 * An axis whose size does not change still takes its (identity) table. */
int mcav_resample_coeffs(int in_size, int out_size, int* ksize_out, int* bounds, int* kk, int kk_capacity);
size_t mcav_image_preprocess_workspace_bytes(int B, int H0, int w);
int mcav_image_preprocess(const unsigned char* src_bhwc, int B, int H0, int W0, int h, int w, const int* hbounds, const int* hkk, int hksize,
                          const int* vbounds, const int* vkk, int vksize, const float* mean3, const float* std3, float* dst_bchw,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Training-time augmentation (monodepth2): mcav_image_preprocess plus a horizontal flip and torchvision's ColorJitter on Pillow images, per
 * frame.  The definition is tests/augment_ref.py.  For frame b with record rec = records[b] and R = the resized uint8 image of
 * mcav_image_preprocess (bit-exact against Pillow's resize):
 *   MCAV_AUG_FLIP:   R = R[:, ::-1]  (equal to Pillow's transpose(FLIP_LEFT_RIGHT) before the resize)
 *   plain[b]       = Normalize(R / 255)
 *   MCAV_AUG_COLOUR: the operations rec.order[0..3] in that order, each uint8 -> uint8 as Pillow; an entry above 3 is skipped
 *     BRIGHTNESS(f) = blend(0, R, f)              SATURATION(f) = blend(L(R), R, f)        (ImageEnhance.Brightness / Color)
 *     CONTRAST(f)   = blend(int(S / n + 0.5), R, f), S = the integer sum of L over the frame as it stands at that point (ImageEnhance.Contrast)
 *     HUE(shift)    = RGB -> HSV (Pillow), H = (H + shift) mod 256, HSV -> RGB (Pillow)   (torchvision F_pil.adjust_hue)
 *     with L(p) = (19595 r + 38470 g + 7471 b + 0x8000) >> 16 and blend(a, b, f) = ImagingBlend in float32.
 *   aug[b]         = Normalize(R / 255)   (equal to plain[b] without MCAV_AUG_COLOUR)
 * records: DEVICE array of B records (the caller repeats a sample's record for its frames).  Unknown flag bits are ignored and hue_shift is
 * taken mod 256, so no record reads or writes out of bounds.  plain, aug: device float [B,3,h,w].  The other arguments and the resample
 * tables as mcav_image_preprocess.  Deterministic: integer sums only (one 64-bit atomic per workgroup), outputs bit-identical from run to
 * run; no host synchronisation, allocation or copy (one hipMemsetAsync of the sums): the call can be captured.  4 launches.
 * Workspace (mcav_image_augment_workspace_bytes, each piece rounded up to 256 bytes): B * H0 * w * 3 + B * h * w * 4 + B * 8 bytes.
 * Returns MCAV_E_INVALID for a null pointer, a non-positive size or B > 65535, MCAV_E_WORKSPACE for a workspace below
 * mcav_image_augment_workspace_bytes(B, H0, h, w); nothing is launched then. */
#define MCAV_AUG_FLIP 1
#define MCAV_AUG_COLOUR 2
#define MCAV_AUG_OP_BRIGHTNESS 0
#define MCAV_AUG_OP_CONTRAST 1
#define MCAV_AUG_OP_SATURATION 2
#define MCAV_AUG_OP_HUE 3
#define MCAV_AUG_OP_NONE 255
typedef struct mcav_augment_record {
    int32_t flags;              /* MCAV_AUG_FLIP | MCAV_AUG_COLOUR */
    uint8_t order[4];           /* MCAV_AUG_OP_* in the order applied (torchvision's random permutation) */
    float brightness;           /* blend factors, float32 as ImagingBlend takes them */
    float contrast;
    float saturation;
    int32_t hue_shift;          /* trunc(hue_factor * 255) mod 256 */
} mcav_augment_record;          /* 24 bytes */
size_t mcav_image_augment_workspace_bytes(int B, int H0, int h, int w);
int mcav_image_preprocess_augment(const unsigned char* src_bhwc, int B, int H0, int W0, int h, int w, const int* hbounds, const int* hkk,
                                  int hksize, const int* vbounds, const int* vkk, int vksize, const float* mean3, const float* std3,
                                  const mcav_augment_record* records, float* plain_bchw, float* aug_bchw, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Oriented 3-D boxes: overlap and batched greedy non-maximum suppression, what follows a detector's head (OpenPCDet / second.pytorch
 * iou3d_nms: boxes_iou_bev, boxes_iou3d, nms_gpu).  The definition is tests/box_ref.py; the arithmetic is csrc/box_math.h.
 *   box      7 float32 (x, y, z, dx, dy, dz, heading): the centre, dx along the heading, the heading a rotation about +z, counter-
 *            clockwise (OpenPCDet's LiDAR frame).  VALID when all seven are finite, 0.001 <= dx, dy, dz <= 1024 and |heading| <= 32
 *            (above 8 pi).  An invalid box has overlap +0.0 with every box, itself included, and is never a candidate.
 *   sincos   box_sincos of csrc/box_math.h: fmaf steps alone, the same bits on the host and the device, at most 1.5625 ulp from the
 *            float64 sine and cosine over every allowed heading
 *   inter    B's centre minus A's first; corners from (cos, sin, half extents); A's quadrilateral clipped against B's four half-planes
 *            in a fixed order (Sutherland-Hodgman; inside is side >= 0 of a fixed fmaf expression, a crossing is strictly opposite
 *            signs, at t = sp / (sp - sq)); at most 8 vertices; half the shoelace sum in a fixed order, clamped to [0, min(area A,
 *            area B)].  +0.0 at once when the centres are further apart than the half-diagonals reach.  No epsilon constants.
 *   iou      bev: inter / (area A + area B - inter); 3d: i3 / (vol A + vol B - i3), i3 = min(inter * max(0, min(top) - max(bottom)), vol A, vol B), the
 *            box spanning z -+ dz / 2.  IEEE division; never above 1.
 * mcav_box_iou: a [na, 7], b [nb, 7] -> out [na, nb] float32 on the device, out[i][j] = iou(a[i], b[j]) in `mode`, every element written.
 * 1 launch (none when na or nb is 0), no workspace, no atomics, no host synchronisation.  Returns MCAV_E_INVALID for a null pointer, an
 * address that is no multiple of 4, a negative na or nb or one above 65535 * 64, or an unknown mode; nothing is launched then. */
#define MCAV_BOX_IOU_BEV 0
#define MCAV_BOX_IOU_3D 1
#define MCAV_NMS_MAX_CANDIDATES 4096
int mcav_box_iou(const float* a, long long na, const float* b, long long nb, int mode, float* out, void* stream);
/* mcav_box_nms: score threshold -> top pre_max -> greedy suppression, per image, over dense device inputs boxes [B, A, 7] float32,
 * scores [B, A] float32 and classes [B, A] int32 (or NULL: one class).
 *   1. Row i of an image is a candidate when its box is valid and score >= score_thresh (a NaN score never is; -0.0 counts as +0.0).
 *   2. The candidates are ordered by score descending, then index ascending; beyond pre_max of them the first pre_max remain.
 *   3. They are walked in that order; one is kept iff no earlier KEPT candidate of the same class has iou > iou_thresh with it
 *      (iou(earlier, later) in `mode`); the walk stops after post_max kept.
 *   4. keep [B, post_max] int32: the kept rows' indices in the order kept, -1 behind the count; num [B] int32: the count;
 *      out_boxes [B, post_max, 7] and out_scores [B, post_max] (each may be NULL): the kept rows as they stand in the inputs, +0.0
 *      behind the count.  One call writes every element of all four.
 * Nothing returns to the host, no allocation, no global atomics (LDS integer counts in the radix select, exact in any order), nothing
 * depends on timing: the call can be captured and two runs give the same bytes.  3 launches: select (one workgroup per image: count,
 * radix select of the cut above pre_max, compaction in index order, an ordering of <= 4096 (key, index) pairs in LDS), mask (64 x 64 tiles
 * of the upper triangle below the candidate count, a row's word is one 64-bit ballot), scan (one wavefront per image, 64 candidates
 * at a time).
 * Workspace (mcav_box_nms_workspace_bytes, 0 for sizes that are refused; scratch of one call, no zero-fill, each piece rounded up to
 * 256 bytes): 4 B + B pre_max (4 + 4 + 80 + 8 ceil(pre_max / 64)) bytes.
 * Returns MCAV_E_INVALID for a null boxes, scores, keep, num or workspace, B outside [1, 65535], A < 1, B * A >= 2^31, pre_max outside
 * [1, MCAV_NMS_MAX_CANDIDATES], post_max outside [1, pre_max], a NaN threshold, an unknown mode, an address that is no multiple of 4 or
 * a workspace address that is no multiple of 16; MCAV_E_WORKSPACE for a short workspace; nothing is launched and no output is touched
 * then. */
size_t mcav_box_nms_workspace_bytes(int B, long long A, int pre_max);
int mcav_box_nms(const float* boxes, const float* scores, const int* classes /* may be null */, int B, long long A, float score_thresh,
                 float iou_thresh, int mode, int pre_max, int post_max, int* keep, int* num, float* out_boxes /* may be null */,
                 float* out_scores /* may be null */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCAV_DEPTH_H */
