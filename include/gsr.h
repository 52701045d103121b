/*
 * include/gsr.h -- C ABI of the MI355X (gfx950) Gaussian rasterizer library libgsr_hip.so.
 *
 * Drop-in boundary.  The reference binds its rasterizer through the Python module
 * `diff_gaussian_rasterization` (call sites: /root/reference/scene/gaussian_model_ht.py:809-880,
 * /root/reference/gaussian_renderer/__init__.py:38-96, /root/reference/scene/gaussian_model.py:935-1009),
 * whose native extension `_C` is an UN-VENDORED submodule (/root/reference/.gitmodules:4-6).  The three entry
 * points a maintainer's FFI for this path would bind are restated here as plain C:
 *
 *   gsr_forward       <- the extension's forward  ("rasterize_gaussians"), invoked by GaussianRasterizer.forward
 *                        as called at gaussian_model_ht.py:871-880; returns what :881-894 unpacks
 *   gsr_backward      <- the extension's backward ("rasterize_gaussians_backward"), reached by loss.backward()
 *                        at /root/reference/trainer/ht3dgs_trainer.py:135; produces the grads consumed at
 *                        gaussian_model_ht.py:718-721 (means2D) and by the Adam groups :275-289
 *   gsr_mark_visible  <- the extension's "mark_visible" (GaussianRasterizer.markVisible; unused by the reference)
 *
 * Rules: extern "C", raw DEVICE pointers and sizes only, no torch types, no exceptions.  Every call is
 * asynchronous on `stream` (a hipStream_t passed as void*) except for one device->host read of the instance
 * count inside gsr_forward.  Return 0 on success, a negative GSR_ERR_* otherwise; gsr_last_error() gives text.
 * All float tensors are binary32, contiguous.  4x4 matrices are read linearly as the reference stores them
 * (transposed, /root/reference/scene/cameras.py:76-98).
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_OK 0
#define GSR_ERR_ARG (-1)
#define GSR_ERR_HIP (-2)
#define GSR_ERR_ALLOC (-3)
#define GSR_ERR_RANGE (-4)

#define GSR_ALLOC_BINNING 0 /* kept by the caller until gsr_backward */
#define GSR_ALLOC_SCRATCH 1 /* may be released (stream-ordered) as soon as gsr_forward returns */

/* Allocator callback: return a device pointer to `bytes` bytes (>=256-byte aligned) or NULL. */
typedef void* (*gsr_alloc_fn)(size_t bytes, int tag, void* user);

/* Batched rendering of INDEPENDENT models in one launch chain (stage A of the reference fits F - 1 single-image models that share
 * nothing, /root/reference/trainer/ht3dgs_trainer.py:697-698, :336-431; each is a chain of ~17 dependent kernels that fill a
 * fraction of the chip).  B models live in ONE parameter store of N Gaussians; model b owns the 128-Gaussian blocks
 * [first_block[b], first_block[b + 1]) -- every model is padded to a multiple of 128 Gaussians (padding = Gaussians that are culled,
 * e.g. opacity logit -30) and N = 128 first_block[B].  With a batch attached:
 *   viewmatrix / projmatrix / campos / points_transform (and those of GsrNextView) are arrays of B entries (16 / 16 / 3 / 12 floats);
 *   out_color is [B,3,H,W], out_depth / out_alpha [B,1,H,W], the upstream gradients of gsr_backward likewise;
 *   d_viewmatrix / d_projmatrix / d_campos / d_points_transform are arrays of B entries;
 *   `image` holds gsr_image_bytes_batched(W, H, B) bytes;  W, H, tanfov, bg, sh_degree, scale_modifier are shared.
 * Every model's image, radii and gradients are bit-identical with rendering it alone: the B images form one tall tile grid
 * (tile id = b T + tile), a tile's list only holds its own model's Gaussians, and one depth sort orders them all.
 * first_block is a HOST pointer (B + 1 entries).  B <= 16.  NULL / B <= 1 = the ordinary single-model call. */
typedef struct GsrBatch {
    int32_t B;
    const int32_t* first_block;
} GsrBatch;

typedef struct GsrForwardArgs {
    int32_t N;           /* Gaussians */
    int32_t M;           /* SH coefficients stored per Gaussian (row stride of shs), e.g. 16 */
    int32_t D;           /* active SH degree 0..3 (raster_settings.sh_degree) */
    int32_t W, H;        /* image_width, image_height */
    int32_t prefiltered; /* accepted, ignored (reference always passes False: gaussian_model_ht.py:820) */
    int32_t debug;       /* accepted, ignored (reference always passes False: gaussian_model_ht.py:821) */
    float scale_modifier, tanfovx, tanfovy;
    const float* means3D;        /* [N,3] */
    const float* scales;         /* [N,3]  or NULL when cov3D_precomp is given */
    const float* rotations;      /* [N,4]  (w,x,y,z) */
    const float* cov3D_precomp;  /* [N,6]  xx,xy,xz,yy,yz,zz or NULL */
    const float* opacities;      /* [N] */
    const float* shs;            /* [N,M,3] or NULL when colors_precomp is given */
    const float* colors_precomp; /* [N,3] or NULL */
    const float* viewmatrix;     /* 16 floats, device */
    const float* projmatrix;     /* 16 floats, device */
    const float* campos;         /* 3 floats, device */
    const float* bg;             /* 3 floats, device */
    float* out_color;            /* [3,H,W] */
    float* out_depth;            /* [1,H,W] */
    float* out_alpha;            /* [1,H,W] */
    int32_t* radii;              /* [N] */
    void* geom;                  /* gsr_geom_bytes(N) bytes, kept until backward */
    void* image;                 /* gsr_image_bytes(W,H) bytes, kept until backward */
    gsr_alloc_fn alloc;          /* called for the R-sized buffers once R is known */
    void* alloc_user;
    /* ---- extension, "next" row f-2 (fused activations; zero/NULL = the reference's calling convention) ---- */
    const float* shs_rest;       /* if non-NULL: shs is _features_dc [N,1,3] and shs_rest is _features_rest [N,M-1,3]
                                    (gaussian_model_ht.py:176-179 concatenates them every call) */
    int32_t raw_params;          /* 1: scales = log-scales, rotations un-normalised, opacities = logits; the
                                    activations of gaussian_model_ht.py:49-65,128-133,187-188 run in-kernel */
    /* ---- extension, "next" row f-4: fused pose action.  NULL = none.  12 floats, row-major 3x4 [R | t], device.
     * Every mean is replaced by R p + t before anything else is computed -- the in-kernel form of
     * `xyz = self.P[k].retr().act(self._xyz.clone())` (gaussian_model_ht.py:135-148): positions move, the Gaussians'
     * own rotations / scales / SH do not, exactly as the reference's get_xyz has it. */
    const float* points_transform;
    /* ---- "prepare in backward" (see GsrNextView): the buffer a preceding gsr_backward filled through
     * GsrBackwardArgs::prepared_out for THIS camera and THESE parameter values.  Then `geom` must be the same pointer (the
     * splat records are its first gsr_geom_bytes(N) bytes), k_preprocess is skipped, and the result is bit-identical to a
     * forward without it.  NULL = ordinary forward.  The buffer is consumed: it also holds the depth sort's scratch, pre-cleared
     * (and for N <= 262 144 with the digit counts already in it) by that backward, and its sort keys are sorted in place --
     * one forward per hand-over. */
    void* prepared;
    const struct GsrBatch* batch; /* NULL = one model (see GsrBatch) */
    /* ---- round 5: the caller's id of the FRAME this render shows (the reference's `viewpoint_camera.uid`, trainer/trainer.py:573;
     * any non-zero number that is the same whenever the same frame is rendered).  0 = none.  Speed only, never the result: the
     * forward blend places its waves by the work each did at the previous render of the same frame ("blend_balance"); with an id
     * that frame is recognised whatever its pose does in between, without one it is recognised by its pose (view matrix AND
     * points_transform within "view_pose_tol_e6" of the previous render's -- the reference keeps an identity camera and moves the
     * points, gaussian_model_ht.py:135-148, and steps the pose after every render, ht3dgs_trainer.py:162-166). */
    int64_t view_id;
    /* ---- round 5: two results the reference's render wrapper derives with a torch launch each (gaussian_model_ht.py:883, :905), written
     * by kernels that hold the values anyway.  NULL = not wanted.
     *   out_color_clamped [3,H,W] (a batch: [B,3,H,W]): clamp(out_color, 0, 1), by the forward blend;
     *   visible [N] bytes: radii > 0, by the preprocess -- NOT written by a forward that takes a `prepared` buffer (no preprocess runs). */
    float* out_color_clamped;
    uint8_t* visible;
    /* ---- version 111: origin of the SH view direction (3 floats, device).  NULL = the module's direction, normalize(posed mean - campos).
     * Set: the direction is normalize(means3D - sh_origin) with the UNtransformed mean (points_transform moves the geometry, not the
     * direction) -- the reference's `convert_SHs_python` render with `view_dependent` (/root/reference/scene/gaussian_model_ht.py:845-865),
     * whose origin is the camera centre in the model's own frame, `get_RT(uid).inverse()[:3, 3]`, detached.  Needs shs; refused
     * (GSR_ERR_ARG) with a batch of B > 1 or a `prepared` buffer.  At sh_degree 0 the colour does not depend on the direction: the
     * result is bit-identical to NULL. */
    const float* sh_origin;
    /* ---- version 116: the RENDER-ONLY call -- an image is asked for and nothing else outlives the call.  0 = the call as above, byte for
     * byte.  Callers that can never reach a backward: the frozen teacher of every virtual-view iteration of train_nonleaf_3DGS_phase1
     * (/root/reference/trainer/ht3dgs_trainer.py:877-883), the eval_nvs loop (:1050-1061), evaluate_on_training_images and render_nvs, all
     * under torch.no_grad() through CF3DGS_Render.render (/root/reference/scene/gaussian_model_ht.py:881-894).  With render_only = 1:
     *   out_color is required; out_depth and out_alpha are given BOTH or NEITHER (one without the other: GSR_ERR_ARG);
     *   out_color_clamped, visible, radii, points_transform, sh_origin, view_id, raw_params, shs_rest, colors_precomp, cov3D_precomp as above;
     *   geom and image may be NULL: the library then takes the splat records (gsr_geom_bytes(N)) and a short image workspace -- the
     *     balanced-placement table and the staged counters, no pixel state -- through alloc(..., GSR_ALLOC_SCRATCH, ...);
     *   the R-sized buffer holds the list and the ranges only (4 R + 8 T bytes) and also comes under GSR_ALLOC_SCRATCH: nothing is
     *     requested under GSR_ALLOC_BINNING, no checkpoint is written, no per-pixel state is kept;
     *   GsrForwardOut: num_rendered = R, binning = NULL, binning_bytes = 0, binning_capacity = 0, forward_flags carries
     *     GSR_FWD_FLAG_RENDER_ONLY -- gsr_backward and gsr_importance_accumulate refuse such flags (GSR_ERR_ARG) before anything is
     *     enqueued;
     *   a batch of B > 1 and `prepared` are refused (GSR_ERR_ARG);
     *   the list cut ("list_cut") is not taken -- its repair pass reads state this call does not keep; the image is the same either way.
     * Capacity hints, speculative binning, the early instance count and its late check, the choice of the list-building route and the
     * balanced placement (its view-cost cache included) are read and updated as by any other forward.  out_color, out_color_clamped,
     * out_depth, out_alpha, radii and visible are bit-identical with the full call's: the blend is the same chain of operations in the
     * same order with the checkpoint stores, the state planes and (without out_depth / out_alpha) the two accumulators left out. */
    int32_t render_only;
} GsrForwardArgs;

#define GSR_FWD_FLAG_RENDER_ONLY ((int64_t)1 << 14) /* GsrForwardOut::forward_flags of a render-only forward */

#define GSR_FWD_FLAG_VIEWS ((int64_t)1 << 15)       /* GsrForwardOut::forward_flags of gsr_forward_views */
#define GSR_MAX_VIEWS 16                            /* views of one gsr_forward_views call (= the models of a GsrBatch) */

typedef struct GsrForwardOut {
    int64_t num_rendered; /* R: (tile, Gaussian) instances */
    void* binning;        /* pointer returned by alloc(GSR_ALLOC_BINNING); pass to gsr_backward */
    size_t binning_bytes;
    int64_t binning_capacity; /* instances the binning buffer was laid out for (>= R when the forward ran speculatively);
                                 pass to gsr_backward together with `binning` */
    int64_t forward_flags;    /* what this forward fixed for its backward (the first checkpointed batch; the render-only bit):
                                 pass to gsr_backward unchanged.  gsr_set_option calls between the two then cannot make the
                                 backward read checkpoints the forward never wrote.  (The bits that once told the blend kernel
                                 variant and the tile -> XCD map keep their place and hold the one value left; flags that
                                 carry another are refused, GSR_ERR_ARG.) */
} GsrForwardOut;

/* Optimizer-in-backward: with raw_params = 1, shs (= _features_dc) + shs_rest given and this struct attached,
 * gsr_backward applies the Adam step of /root/reference/scene/gaussian_model_ht.py:275-289 (torch.optim.Adam, no
 * amsgrad / weight decay; ht3dgs_trainer.py:159-166 calls step() right after backward()) to the six parameter tensors
 * IN PLACE inside the per-Gaussian backward kernel, instead of writing their gradients: the gradient never makes
 * the round trip through HBM (2180 -> ~1480 bytes per Gaussian for backward + optimizer).  The parameter pointers of
 * GsrBackwardArgs (means3D, shs, shs_rest, opacities, scales, rotations) are then written through; d_means3D,
 * d_opacities, d_shs, d_shs_rest, d_scales, d_rotations are ignored (may be NULL); d_means2D is still produced
 * (densification statistics, gaussian_model_ht.py:718-721).  Group order of lr / exp_avg / exp_avg_sq:
 * 0 xyz, 1 f_dc, 2 f_rest, 3 opacity, 4 scaling, 5 rotation.  `step` is the 1-based step count.
 * exp_avg[2] == exp_avg_sq[2] == NULL: the f_rest group is left alone -- no read or write of its 45 floats of parameters and 90 of
 * moments per Gaussian, three quarters of the update's traffic.  Accepted only for a render at sh_degree 0 that prepares no view
 * of a higher degree (the group's gradient is then identically zero), and CORRECT only if the caller knows the group's moments
 * to be all zero: Adam with g = m = v = 0 leaves parameter and moments unchanged bit for bit (0 / (0 + eps) = 0), so skipping it
 * is the same update.  That is a model's state from its creation until its first step at degree >= 1 -- all of stage A and the
 * first 1 000 iterations of every leaf (gaussian_model_ht.py:68, :193-195); optim.FusedAdam tracks it. */
typedef struct GsrFusedAdam {
    float beta1, beta2, eps;
    int32_t reserved;
    int64_t step;
    float lr[6];
    float* exp_avg[6];
    float* exp_avg_sq[6];
    int32_t step_lag[6];    /* round 4: group q is at step `step - step_lag[q]` (its bias corrections use that count); all zero =
                             * the six groups in lockstep.  The reference drops a group's update when its tensor is replaced
                             * between backward() and optimizer.step() (opacity reset: gaussian_model_ht.py:468-474,
                             * ht3dgs_trainer.py:153-160), after which that group's count stays behind the others'. */
    /* round 4, DEFERRED application: when a group's three pointers are set, its updated parameter rows and moments are written
     * THERE instead of in place (inputs untouched), and the caller adopts them -- swaps the buffers -- when its `optimizer.step()`
     * runs, or drops them when the step never comes (the reference's trainer densifies between backward() and step() and then
     * steps nothing: ht3dgs_trainer.py:137-160).  All NULL = in place.  Not together with next_view. */
    float* param_out[6];
    float* exp_avg_out[6];
    float* exp_avg_sq_out[6];
} GsrFusedAdam;

/* "Prepare in backward" (extension f-2, with fused_adam only).  Training renders the same parameters again right after
 * their update; when the caller knows the NEXT camera at backward time, the per-Gaussian backward kernel -- which holds
 * each Gaussian's freshly updated parameters in registers / LDS -- also runs the forward preprocess of that next render
 * (projection, tile test, SH colour, sort keys) and leaves the result in `prepared_out`; the next gsr_forward takes it
 * through GsrForwardArgs::prepared and skips its preprocess kernel: no second read of the 236 bytes per Gaussian, and
 * the ~2 400 VALU instructions per wave of the preprocess hide under the HBM time of the backward kernel.
 * Needs raw_params, shs + shs_rest with M = 16 stored coefficients at any active degree D = 0..3 (gsr_prepare_supported) --
 * the reference's models store 16 coefficients from the start and raise the active degree once per 1 000 iterations
 * (/root/reference/scene/gaussian_model_ht.py:68,193-195); GsrNextView::D is this render's degree or one above it (an
 * `oneupSHdegree` between the two steps keeps the hand-over).  The caller guarantees that the parameters are not modified
 * between this backward and that forward. */
typedef struct GsrNextView {
    int32_t W, H, D;
    float scale_modifier, tanfovx, tanfovy;
    const float *viewmatrix, *projmatrix, *campos; /* device, as in GsrForwardArgs */
    const float* points_transform;                  /* device, 12 floats, or NULL */
} GsrNextView;

/* Per-iteration densification statistics, folded into the per-Gaussian backward kernel (it holds the screen-space gradient in
 * registers).  What the reference's train_step does after every backward while iteration < densify_until_iter
 * (/root/reference/trainer/ht3dgs_trainer.py:137-147, /root/reference/scene/gaussian_model_ht.py:718-721), for the visible
 * Gaussians (radii > 0):  max_radii2D = max(max_radii2D, radii);  xyz_gradient_accum += |d_means2D[:, :2]|;  denom += 1.
 * radii = the forward's int32 output; the three float arrays hold N elements each and are updated in place. */
typedef struct GsrDensifyStats {
    const int32_t* radii;
    float* xyz_gradient_accum;
    float* denom;
    float* max_radii2D;
} GsrDensifyStats;

/* ---- version 115: the FROZEN CALL -- pose and camera gradients of a model that does not move.
 * The reference optimises six pose numbers against fixed Gaussians in stage A's pose phase (train_relative_pose,
 * /root/reference/trainer/ht3dgs_trainer.py:307-335, after training_setup_fix_position / fix_position,
 * /root/reference/scene/gaussian_model_ht.py:321-343, 235-248), in train_pose_only (ht3dgs_trainer.py:916-963) and in the test-time
 * pose fit of eval_nvs (:1018-1042): nobody reads a per-Gaussian gradient there.  A gsr_backward call is FROZEN when
 *     fused_adam == NULL,
 *     every per-Gaussian gradient pointer is NULL (d_means3D, d_opacities, d_colors_precomp, d_shs, d_shs_rest, d_scales, d_rotations,
 *     d_cov3D_precomp), and
 *     at least one of d_viewmatrix, d_projmatrix, d_campos, d_points_transform is set.
 * It runs the same prologue and backward blend, then a variant of the per-Gaussian kernel that keeps what feeds the camera and transform
 * gradients and leaves out the chain rules and the 62 floats per Gaussian of the parameter gradients; no buffer for them is needed.
 * With the same blend result (option "deterministic_backward") its outputs are bit-identical with those of the full call.
 * d_means2D is OPTIONAL in a frozen call: written when non-NULL, never required.  Accepted with raw or activated parameters, shs alone or
 * shs + shs_rest, colors_precomp, cov3D_precomp, sh_origin, grad_depth / grad_alpha, any D <= 3 with any stored M, a GsrBatch of B <= 16.
 * Refused with GSR_ERR_ARG (gsr_last_error() names the rule), before anything is enqueued on the stream:
 *     a frozen call with next_view / prepared_out (they need fused_adam);
 *     a frozen call with densify_stats (fed by the gradients it leaves out);
 *     d_means3D == NULL while another per-Gaussian gradient pointer is set (without fused_adam they come together or not at all);
 *     every per-Gaussian gradient pointer NULL and no camera / transform output either (nothing to compute). */
typedef struct GsrBackwardArgs {
    int32_t N, M, D, W, H;
    float scale_modifier, tanfovx, tanfovy;
    const float *means3D, *scales, *rotations, *cov3D_precomp, *opacities, *shs, *colors_precomp;
    const float *viewmatrix, *projmatrix, *campos, *bg;
    const void* geom;    /* from forward */
    const void* image;   /* from forward */
    void* binning;       /* from forward.  WRITTEN by gsr_backward (round 4): the backward blend's work-item lists and queue heads live in
                          * this buffer, so two backwards over the SAME forward output must not run concurrently (serialise them on one
                          * stream); a repeated backward on one stream is fine -- the lists are rebuilt by every call */
    int64_t num_rendered;
    const float* grad_color; /* [3,H,W] or NULL */
    const float* grad_depth; /* [1,H,W] or NULL */
    const float* grad_alpha; /* [1,H,W] or NULL */
    float* d_means3D;        /* [N,3]; NULL together with every other per-Gaussian gradient pointer = frozen call (above) */
    float* d_means2D;        /* [N,3]  (d/d ndc x, d/d ndc y, 0): gaussian_model_ht.py:718-721; may be NULL in a frozen call */
    float* d_opacities;      /* [N] */
    float* d_colors_precomp; /* [N,3] or NULL */
    float* d_shs;            /* [N,M,3] or NULL */
    float* d_scales;         /* [N,3] or NULL */
    float* d_rotations;      /* [N,4] or NULL */
    float* d_cov3D_precomp;  /* [N,6] or NULL */
    void* scratch;           /* gsr_backward_scratch_bytes(N) bytes */
    /* ---- extension f-2: same meaning as in GsrForwardArgs; gradients are returned w.r.t. the raw parameters ---- */
    const float* shs_rest;
    float* d_shs_rest;       /* [N,M-1,3] when shs_rest is given (then d_shs is [N,1,3]) */
    int32_t raw_params;
    /* ---- camera gradients (north_star: dL/dviewmatrix; BASELINE config 5).  NULL = not wanted.  Entries follow
     * the linear storage of the inputs.  projmatrix row 2 (clip z) does not influence the render: its grad is 0. */
    float* d_viewmatrix;     /* 16 */
    float* d_projmatrix;     /* 16 */
    float* d_campos;         /* 3 */
    /* ---- optimizer-in-backward (extension f-2, see GsrFusedAdam below).  NULL = plain backward. */
    const struct GsrFusedAdam* fused_adam;
    /* ---- fused pose action (f-4): the transform given to the forward, and where dL/d(transform) (12 floats, same
     * layout) goes; d_means3D is then the gradient w.r.t. the UNtransformed means (R^T dL/dp'). */
    const float* points_transform;
    float* d_points_transform;
    int64_t binning_capacity; /* GsrForwardOut::binning_capacity of the forward (0 = num_rendered) */
    int64_t forward_flags;    /* GsrForwardOut::forward_flags of the forward (0 = round-1 caller: process-wide options) */
    const struct GsrNextView* next_view; /* NULL = none; otherwise prepared_out must point at gsr_prepared_bytes(N) bytes */
    void* prepared_out;
    const struct GsrDensifyStats* densify_stats; /* NULL = none */
    const struct GsrBatch* batch;                 /* the forward's batch (NULL = one model) */
    /* version 111: the forward's sh_origin (see GsrForwardArgs).  The colour's share of the mean gradient is then w.r.t. the
     * untransformed mean: it is added to d_means3D after the R^T chain of points_transform and reaches none of d_points_transform,
     * d_campos, d_viewmatrix.  Needs shs; refused (GSR_ERR_ARG) with a batch of B > 1 or next_view. */
    const float* sh_origin;
    /* version 117: the forward's retire table and step (see gsr_forward_retire; ht3dgs_trainer.py:299-300).  Needs fused_adam.
     *   The Adam update of step s runs for model b exactly when retired_at[b] == 0 || retired_at[b] >= s -- the update of the step at which a
     *   model retires still applies, as the reference steps its optimizer before it breaks.  A skipped model's parameters and both moments
     *   stay untouched bit for bit (its blocks issue none of their parameter or moment streams), its d_means2D rows, d_points_transform and
     *   camera entries are exact zeros.
     *   The hand-over for the next render (next_view / prepared_out) is written CULLED for model b when retired_at[b] != 0 &&
     *   retired_at[b] < s + 1: the forward that consumes the buffer sees the model as the render of step s + 1 must.
     * Refused (GSR_ERR_ARG, before anything is enqueued): a table without fused_adam (the frozen call included), with deferred application
     * (GsrFusedAdam::param_out), with densify_stats, or with retire_step < 1. */
    const int32_t* retired_at;
    int64_t retire_step;
} GsrBackwardArgs;

size_t gsr_geom_bytes(int32_t N);
size_t gsr_image_bytes(int32_t W, int32_t H);
size_t gsr_image_bytes_batched(int32_t W, int32_t H, int32_t B); /* image workspace of a batched render (GsrBatch) */
/* byte offset inside the image workspace of the per-tile uint32 "instances actually staged" counters that
 * the forward blend writes (their sum is R_eff of the roofline accounting) */
size_t gsr_image_staged_offset(int32_t W, int32_t H);
size_t gsr_forward_scratch_bytes(int32_t N);
size_t gsr_binning_bytes(int64_t R, int32_t W, int32_t H);
/* upper bound of what the forward asks its allocator for (GSR_ALLOC_SCRATCH): sized for 32-bit tile keys, which images
 * above 65 536 tiles use; smaller images carry 16-bit keys and ask for 4 R bytes less */
size_t gsr_binning_scratch_bytes(int64_t R);
size_t gsr_backward_scratch_bytes(int32_t N);
size_t gsr_prepared_bytes(int32_t N);                       /* "prepare in backward": size of the hand-over buffer */
size_t gsr_prepared_radii_offset(int32_t N);                /* where its int32 radii[N] start: a forward given `radii` = that
                                                               address uses them in place instead of copying them out */
int gsr_prepare_supported(int32_t M, int32_t D, int32_t raw_params); /* 1 when gsr_backward can prepare the next view */

int gsr_forward(const GsrForwardArgs* args, GsrForwardOut* out, void* stream);
/* ---- version 117: the forward of a launch chain with a RETIRE TABLE (stage A's per-model early exit, decided and applied on the device).
 * The reference leaves a single-image model's loop at the first iteration past 500 where that model's PSNR exceeds 35 dB
 * (train_single_image_3DGS, /root/reference/trainer/ht3dgs_trainer.py:299-300), AFTER that iteration's optimizer.step().  retired_at: B int32
 * entries on the device (one entry with batch == NULL), 0 = active, otherwise the 1-based step at which gsr_batch_retire retired the model;
 * retire_step = the step s of THIS call (>= 1, the counter GsrFusedAdam::step receives).  retired_at == NULL: gsr_forward itself, byte for byte
 * (gsr_forward(args, out, stream) IS gsr_forward_retire(args, NULL, 0, out, stream)).
 *   The render of step s CULLS model b exactly when retired_at[b] != 0 && retired_at[b] < s: every Gaussian of the model gets radius 0,
 *   `visible` 0 and no instance; its image is the background, its depth and alpha planes are 0, and nothing downstream of it can carry a
 *   gradient (the loss kernels are untouched: a reported loss sum still contains the retired images' terms, background against target).
 *   A forward that takes a `prepared` buffer does not read the table: the backward that filled the buffer applied the same test
 *   (GsrBackwardArgs::retired_at).
 * The table travels beside GsrForwardArgs, not in it: that struct keeps its version-116 layout, which tests/test_render_only_cpu.py pins
 * (render_only is its last field); GsrBackwardArgs carries the table as appended fields.  gsr_importance_accumulate takes a GsrForwardArgs and
 * therefore no table: the pass cannot be given one.
 * Refused (GSR_ERR_ARG, before anything is asked for or enqueued): a table with args->render_only, or with retire_step < 1. */
int gsr_forward_retire(const GsrForwardArgs* args, const int32_t* retired_at, int64_t retire_step, GsrForwardOut* out, void* stream);
int gsr_backward(const GsrBackwardArgs* args, void* stream);
int gsr_mark_visible(int32_t N, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* ---- version 113: merge-time colour importance of one view WITHOUT a backward.
 * Replaces, per view, the body of `HTGaussianTrainer.calc_importance` (/root/reference/trainer/ht3dgs_trainer.py:1427-1462: render,
 * `rendering.sum().backward()` on the clamped image, `|grad|` of _features_dc / _features_rest through the hooks of :1436-1437).
 * With L = sum clamp(image, 0, 1) the gradient of SH coefficient k, channel c of Gaussian n in one view is
 *     dL/dSH[n,k,c] = basis_k(dir_n) * [colour_{n,c} not clamped at 0] * S[n,c],
 *     S[n,c] = sum over pixels of alpha T * [0 <= out_color_c(pixel) <= 1],
 * and alpha T is the weight the FORWARD blend forms for every contribution it takes; S >= 0, so the per-view |grad| is
 * |basis_k| * gate * S.  The pass walks the forward's tile lists a second time in forward order with its out_color in hand (the same
 * visit code as the forward blend: the same contributions) and sums S; a short per-Gaussian kernel then adds |basis_k| gate S to
 * acc[n,k,c] for k < (D+1)^2.  No checkpoint, no back-to-front replay, no geometry gradient, no autograd.
 *   fwd / out  the arguments and the result of the gsr_forward just run on the same stream.  Read: geom, image, binning, out_color,
 *              means3D, campos, points_transform, sh_origin.  Written: acc and scratch only -- an ordinary gsr_backward of that
 *              forward afterwards is still valid.
 *   acc        [N,M,3] float, += (M = fwd->M, the stored coefficients).  Rows of Gaussians whose three sums are zero in this view are
 *              neither read nor written; coefficients k >= (D+1)^2 are never touched.
 *   scratch    gsr_importance_scratch_bytes(N) bytes; cleared by the pass itself (an asynchronous fill on the stream).
 * Raw or activated parameters, shs alone or shs + shs_rest, cov3D_precomp, points_transform, sh_origin, any D <= 3 with any stored
 * M >= (D+1)^2.  Refused (GSR_ERR_ARG): colors_precomp (no SH) and a batch of B > 1.  Float atomics: the sums of two runs may differ in
 * the last bits.  Profile stages: "importance_blend", "importance_finish". */
size_t gsr_importance_scratch_bytes(int32_t N);
int gsr_importance_accumulate(const GsrForwardArgs* fwd, const GsrForwardOut* out, float* acc /* [N,M,3], += */, void* scratch,
                              void* stream);

/* ---- version 123: V VIEWS OF ONE MODEL in one launch chain, and the colour importance over them.
 * gsr_forward_views is the full forward of ONE model under V cameras, 1 <= V <= GSR_MAX_VIEWS.  GsrForwardArgs is unchanged (the count
 * travels beside it, as the retire table of gsr_forward_retire does); with Npad = 128 ceil(N / 128) -- the caller does not pad, any N >= 1:
 *   viewmatrix / projmatrix / campos are arrays of V entries (16 / 16 / 3 floats); points_transform and sh_origin, when given, are arrays
 *     of V entries (12 / 3 floats); W, H, tanfov*, bg, D and scale_modifier are shared;
 *   record v Npad + n is Gaussian n under camera v; the records n >= N of each view are culled records (radius 0, no tile);
 *   geom holds gsr_geom_bytes_views(N, V) bytes, image gsr_image_bytes_batched(W, H, V) bytes; radii and visible are [V Npad];
 *   out_color and out_color_clamped are [V,3,H,W], out_depth and out_alpha [V,1,H,W].
 * The preprocess reads the model's ONE set of parameter rows for every view (a GsrBatch would need V copies of them); behind it the chain
 * is the one a GsrBatch with first_block = {0, nb, 2 nb, ...} takes: every view's image, radii and visibility bytes are bit-identical with
 * rendering that view alone, and the list-building routes, the early instance count, capacity hints, speculative binning and the balanced
 * placement behave as a batched forward of V images treats them.  V = 1 is served: one view through the same front.
 * forward_flags carries GSR_FWD_FLAG_VIEWS: gsr_backward and the single-view gsr_importance_accumulate refuse such flags (GSR_ERR_ARG)
 * before anything is enqueued -- the backward over a views forward is gsr_backward_views (version 124, below), the frozen call only.
 * Refused before a device is touched, the rule in gsr_last_error(): V outside [1, 16]; a->batch set; `prepared`; `render_only`;
 * V Npad >= 2^31 (GSR_ERR_RANGE).  colors_precomp IS served by the forward.
 *
 * gsr_importance_accumulate_views is gsr_importance_accumulate over such a forward: ONE walk of the V T tiles into S[V Npad] (float
 * atomics, as in the single-view pass) and ONE finishing launch that, per Gaussian n, adds |basis_k(dir_{n,v})| gate S[v Npad + n] to
 * acc[n,k,:] for v = 0 .. V-1 IN THAT ORDER -- the order in which V single-view calls add into acc -- with view v's campos,
 * points_transform and sh_origin and the colour gates of record v Npad + n.  A view whose three sums are zero is skipped; a row whose sums
 * are zero in every view is neither read nor written.  acc is [N,M,3] (the MODEL's rows); scratch holds
 * gsr_importance_scratch_bytes_views(N, V) bytes.  Refused as by the single-view entry (colors_precomp, render-only flags), plus flags
 * without GSR_FWD_FLAG_VIEWS and the V rules above. */
size_t gsr_geom_bytes_views(int32_t N, int32_t V);
int gsr_forward_views(const GsrForwardArgs* args, int32_t V, GsrForwardOut* out, void* stream);
size_t gsr_importance_scratch_bytes_views(int32_t N, int32_t V);
int gsr_importance_accumulate_views(const GsrForwardArgs* fwd, int32_t V, const GsrForwardOut* out, float* acc /* [N,M,3], += */,
                                    void* scratch, void* stream);

/* ---- version 124: the FROZEN CALL over V views of one model (fitting V poses against a model that does not move).
 * gsr_backward_views is the frozen call of gsr_backward (camera and transform gradients alone) over the output of a gsr_forward_views of the
 * same N, V, cameras and transforms.  GsrBackwardArgs keeps its layout; the count travels beside it.  N is the MODEL's size;
 *   viewmatrix / projmatrix / campos, and points_transform / sh_origin when given, are arrays of V entries, as in the forward;
 *   grad_color is [V,3,H,W], grad_depth and grad_alpha [V,1,H,W], any subset;
 *   geom, image, binning, num_rendered, binning_capacity and forward_flags come from the forward; scratch holds
 *     gsr_backward_scratch_bytes_views(N, V) bytes;
 *   outputs, any subset, at least one: d_viewmatrix [V,16], d_projmatrix [V,16], d_campos [V,3], d_points_transform [V,12]; optionally
 *     d_means2D [V Npad,3] -- record v Npad + n is Gaussian n under view v, the rows n >= N are written as zeros.
 * Nothing is summed across views: every view's outputs are what a single-view gsr_forward + frozen gsr_backward of that view gives, the
 * same bits under the deterministic_backward option.  The per-Gaussian kernel reads the model's ONE set of parameter rows; a view's padding
 * records read no parameter row.  Accepted: whatever the single-view frozen call accepts (raw or activated parameters, shs alone or shs +
 * shs_rest, colors_precomp, cov3D_precomp, sh_origin, any D <= 3 with any stored M).  Counted once by the "frozen_backward_calls" counter.
 * Refused with GSR_ERR_ARG before anything is enqueued or a device is touched, the rule in gsr_last_error(): V outside [1, 16];
 * V Npad >= 2^31 (GSR_ERR_RANGE); forward_flags without GSR_FWD_FLAG_VIEWS or with the render-only flag; any per-Gaussian gradient pointer
 * or fused_adam (a backward over views serves the frozen call only: a full backward over views is not served); next_view / prepared_out;
 * densify_stats; retired_at; batch; no camera or transform output at all; a missing workspace pointer.  gsr_backward itself keeps refusing
 * the flags of a views forward. */
size_t gsr_backward_scratch_bytes_views(int32_t N, int32_t V);
int gsr_backward_views(const GsrBackwardArgs* args, int32_t V, void* stream);

const char* gsr_last_error(void);
/* 100 * major + minor.  110 (round 6): GsrForwardArgs ends with view_id, out_color_clamped, visible (appended in round 5 under
 * version 100: a caller compiled against a shorter struct must be rebuilt -- check gsr_version() >= 110 AND
 * gsr_struct_bytes(0) == sizeof(GsrForwardArgs), gsr_struct_bytes(1) == sizeof(GsrBackwardArgs) at start-up).
 * 111: GsrForwardArgs and GsrBackwardArgs end with sh_origin.
 * 112: the depth term of the loss (gsr_depth_loss_*); no struct changed.
 * 113: gsr_importance_accumulate / gsr_importance_scratch_bytes; no struct changed.
 * 114: the depth term on a stack of planes (gsr_depth_loss_*_batched); no struct changed.
 * 115: the frozen call of gsr_backward (camera / transform gradients alone, see GsrBackwardArgs); no struct changed.
 * 116: GsrForwardArgs ends with render_only (the render-only call).
 * 117: the retire table: gsr_forward_retire, GsrBackwardArgs ends with retired_at, retire_step, gsr_batch_retire; GsrForwardArgs unchanged.
 * 118: gsr_depth_to_points, gsr_voxel_scratch_bytes, gsr_voxel_down_sample; no struct changes (gsr_struct_bytes as in 117).
 * 119: gsr_camera_from_pose, gsr_pose_virtual_view; no struct changes.
 * 120: gsr_resize_plan, gsr_resize_apply, gsr_resize_scratch_bytes, gsr_resize_plan_bytes (GsrResizeTensor is new); no existing struct changes.
 * 121: gsr_select_scratch_bytes, gsr_select_smallest, gsr_merge_apply (GsrMergeTensor is new); no existing struct changes.
 * 122: gsr_resize_plan_batched, gsr_resize_apply_batched, gsr_resize_scratch_bytes_batched (GsrResizeBatch and GsrResizeBatchTensor are
 *      new); no existing struct or entry changes.
 * 123: gsr_forward_views, gsr_geom_bytes_views, gsr_importance_accumulate_views, gsr_importance_scratch_bytes_views
 *      (GSR_FWD_FLAG_VIEWS); no struct changes.
 * 124: gsr_backward_views, gsr_backward_scratch_bytes_views, gsr_pose_step_many; no struct changes. */
int gsr_version(void);
size_t gsr_struct_bytes(int32_t which); /* 0 GsrForwardArgs, 1 GsrBackwardArgs, 2 GsrForwardOut; anything else 0 */

/* Process-wide knobs (value 0 = default unless stated; the defaults and accepted ranges are those of csrc/options.h, which a call
 * into the library reads once, on entry: setting an option from another thread never changes a call that is under way):
 *   "blend_fwd_ppt"        forward blend kernel: 0 or 7 = one wave per 8x8 sub-tile, finished pixels encoded in the sign of T,
 *                          instances the sub-tile cannot see skipped by reach bits -- the only forward blend, so setting it changes
 *                          nothing.  Any other value is refused (the A/B kernels rounds 1-4 selected with 1-5 left the tree in
 *                          round 5, the kernel without reach bits that 6 selected after them).  bench.py --fwd-ppt passes its value
 *                          on without looking at the return code: with 6 it now measures the default
 *   "blend_bwd_ppt"        backward blend kernel: 0 or 2 = two pixels per lane, packed math, two waves per tile -- the only backward
 *                          blend, so setting it changes nothing.  Any other value is refused (the one-pixel-per-lane kernel that 1
 *                          selected left the tree)
 *   "ab_variants"          query kept for callers of the round-4 ABI: always returns 0 (no A/B kernels in the library)
 *   "sort_algo"            2 = onesweep, the only sort of the library, so setting it changes nothing.  Any other value is refused (the
 *                          histogram + scan + scatter sort that 0 and 1 selected left the tree).  bench.py --sort-algo passes its
 *                          value on without looking at the return code: with 0 or 1 it now measures the default
 *   "bwd_split"            1 = the backward of a tile is ONE work item (off); anything else (default 0) = one item per 128-instance
 *                          batch beyond the first "ckpt_first" (default 1) batches, each resuming from the per-pixel checkpoint the
 *                          forward leaves at every 128-instance boundary.  (Round 4: the items are listed by k_bwd_prologue and
 *                          replayed by persistent workgroups; up to round 3 the value was the number of workgroups per tile.)
 *   "depth_sort9"          1 (default) = depth sort of models above "prep_hist_max_n" Gaussians in THREE 9-bit passes over the 27 bits
 *                          of (key - bits(0.2f)): depths between the near plane and 13 107 units; a visible Gaussian beyond that
 *                          makes the forward sort again on all 32 bits (counter "depth_window_resorts") and keeps that caller on
 *                          the four 8-bit passes; 0 = always four 8-bit passes.  Same order either way
 *   "direct_binning"       1 (default) = the per-tile lists are built by direct placement -- per-chunk tile histograms over the
 *                          depth-ordered Gaussians, column scans, one wave per chunk that places every (Gaussian, tile) pair at
 *                          its final position -- on frames of up to 4 096 tiles; 0 = emit + stable tile sort + ranges (what larger
 *                          frames always take).  Same list, bit for bit
 *   "tile_sort"            1 (default) = where the direct binning runs on a single render AND the caller's tile lists are short (at most
 *                          "tile_sort_max_avg" pairs per tile on average, by the caller's last instance count), the global depth sort is
 *                          left out: the binning walks the Gaussians in index order, places (depth key, Gaussian) pairs, and one
 *                          workgroup per tile sorts its segment by key, stable; 2 = wherever the direct binning runs; 0 = never.
 *                          Same list, bit for bit (equal keys stay in index order, as under the stable global sort)
 *   "tile_sort_max_avg"    (default 700) see "tile_sort"
 *   "blend_balance"        1 (default) = the forward blend places its sub-tile waves by the visits each took at the previous
 *                          render of the same frame (device-side cache of 128 frames per frame size, least recently used out; a
 *                          frame is recognised by GsrForwardArgs::view_id or, without one, by its pose; single renders);
 *                          0 = dispatch order = tile order.  Same image either way
 *   "small_sort9"          (default 1) smallest model for which a forward that runs its own preprocess sorts its depth keys in three
 *                          9-bit passes over the 27-bit window instead of four 8-bit ones (it launches a digit histogram either way);
 *                          0 = only models above 262 144 Gaussians.  Same order either way (a depth beyond the window is detected
 *                          and sorted again on all 32 bits)
 *   "list_cut"             1 (default) = for models of at least "list_cut_min_n" Gaussians (default 2 000 000: where it was measured to pay;
 *                          2 = whatever the size), on the plain direct-binning route (frames of up to 4 096 tiles behind the global depth sort,
 *                          single renders, "blend_balance" on) the tile lists are WRITTEN only up to where the tiles
 *                          stopped at the previous render of the same frame (the frame is recognised as for "blend_balance"; a tile
 *                          remembers the view depth of the last instance any of its four waves staged, x (1 + "list_cut_margin_e3" /
 *                          1000), rounded up to a chunk of the depth order).  One cut for the frame -- the chunk behind which at
 *                          most "list_cut_deep" tiles' cuts lie; the chunks up to it are scattered as ever, for every tile -- and
 *                          the few deeper tiles are served one by one in the chunks behind it.  Counts, scans, tile bases, R and
 *                          every pair's position are the full binning's; the blends get the end of the valid prefix as the range
 *                          end.  Verified and repaired on the device, never by the host: a wave that runs out of a cut list with a
 *                          live pixel flags its tile, and two launches that follow every such render -- the flagged tiles' left-out
 *                          pairs, the blend over the flagged tiles' full lists -- find nothing to do otherwise.  Image, radii,
 *                          every pixel's contributors, checkpoints and all gradients are bit-identical to full lists; ranges[t].y
 *                          and the list words behind it are what differ (gsr_debug_read_binning returns the valid prefixes).
 *                          0 = full lists (gsr_debug_list_cut_stats)
 *   "list_cut_margin_e3"   (default 50), "list_cut_deep" (default 8): see "list_cut"
 *   "early_r"              1 (default) = the host learns the instance count from the preprocess's per-block sums, published by
 *                          the depth sort's first kernel, instead of from the scan behind sort + tile counts; 0 = from the scan.
 *                          The scan still reports its own total and the sorts' give-up counter into spare words of the pinned slot;
 *                          the next gsr_forward that takes the slot (waiting for the report if it must) and every gsr_backward (if
 *                          it has arrived) hold the early values against them and FAIL (GSR_ERR_HIP) on a difference: a forward
 *                          whose count or sort went wrong is reported by the next call into the library, not never
 *                          (counters "late_checks", "late_mismatches"; "debug_late_bias": tests, falsifies the next remembered count)
 *   "view_pose_tol_e6"     (default 2000 = 2e-3) without a view id a render belongs to the cached frame whose view matrix and
 *                          points_transform are within this, x 1e-6, of its own in every entry (the nearest such frame)
 *   "tile_map"             how tiles are dealt to the eight XCDs: 2 = 2x2 blocks of tiles round-robin, the only map of the library, so
 *                          setting it changes nothing.  Any other value is refused (the single tiles round-robin that 1 selected and
 *                          the contiguous band of tiles per XCD that 0 selected left the tree).  bench.py --tile-map passes its
 *                          value on without looking at the return code: with 0 or 1 it now measures the default
 *   "speculative_binning"  1 (default) = R-dependent stages launched against a capacity, R read back late;
 *                          0 = read R, then launch
 *   "binning_capacity_hint" capacity of the NEXT forward, one shot (tests: force the overflow re-run).  The regular hints
 *                          are kept per caller -- (device, image size, half-octave bucket of N) -- so models of different
 *                          size alternating on one process (teacher / student, stage-A models) do not disturb each other
 *   "reset_speculation"    forget every capacity hint and zero the counters of gsr_get_counter
 *   "view_cache_reset"     (tests) every per-frame cache of the current device forgets its frames: the balanced placement's visit
 *                          counts, the list cut's remembered depths, the counters of gsr_debug_view_cache_stats /
 *                          gsr_debug_list_cut_stats (synchronises the device)
 *   "deterministic_backward" 1 = debug mode: the blend backward writes every (tile, Gaussian) partial gradient to its own slot and
 *                          a second kernel sums each Gaussian's slots in list order, in float64; several times slower.  The
 *                          default adds the same float32 parts with float64 atomics in arrival order, and those sums are exact
 *                          (order-independent) while the parts' exponent span plus log2(count) fits in 29 bits: the default gives
 *                          the same bits as this mode apart from rare rounding-boundary flips of inexact sums
 *   "profile"              1 = HIP events around every stage on the caller's stream (an event pair costs ~10 us of stream
 *                          bubble per stage), 2 = only the forward blend kernel is timed, through the start / stop timestamps of
 *                          its own dispatch (hipExtLaunchKernelGGL: still ~11 us of idle queue around the launch), 3 = as 2 on
 *                          every THIRD forward (bench.py's timed region: all of eight rotating views get sampled)
 *   "emit_hist"            1 (default) = the emission kernel counts the tile sort's digits itself (speculative flow); 0 = a
 *                          histogram kernel in front of the sort's passes.  Same lists either way (A/B and tests)
 *   "prep_hist_max_n"      "prepare in backward": up to this many Gaussians (default 262 144) the per-Gaussian backward kernel
 *                          also counts the next depth sort's digits.  Read by BOTH the backward that fills a hand-over buffer
 *                          and the forward that consumes it: do not change it between the two
 *   "poll_iters"           bound of gsr_forward's busy-wait on the pinned instance-count word, in units of ~50 ns (default
 *                          400 000 = 20 ms; past it the call waits with hipStreamSynchronize, which also reports a faulted
 *                          device); 0 = no polling: hipStreamSynchronize at once */
int gsr_set_option(const char* name, int value);
/* Monotonic counters: "spec_forwards" (forwards launched against a capacity), "spec_overflows" (of those, how many had to
 * re-run the binning because R exceeded the capacity), "exact_forwards" (read-then-launch forwards), "spec_callers"
 * (distinct (device, size, N bucket) entries); host-side time accounting: "forward_calls" / "forward_ns" (wall time inside
 * gsr_forward) / "forward_wait_ns" (the part of it spent waiting for the instance count) and "backward_calls" / "backward_ns" --
 * (forward_ns - forward_wait_ns + backward_ns) / calls is what the launching thread works per forward + backward.  -1 for an
 * unknown name. */
int64_t gsr_get_counter(const char* name);   /* + "blend_bwd_resident": workgroups of the backward blend the device holds at once; "depth_window_resorts";
                                                "frozen_backward_calls": gsr_backward calls that took the frozen route (GsrBackwardArgs) */
/* Debug / test hook: copy the per-tile ranges (T x {begin, end} uint32) and the (tile, depth, id)-ordered Gaussian-id list
 * (num_rendered uint32) out of a forward's binning buffer into device buffers of the caller (either may be NULL). */
int gsr_debug_read_binning(const void* binning, int64_t binning_capacity, int64_t num_rendered, int32_t W, int32_t H,
                           uint32_t* ranges_out, uint32_t* list_out, void* stream);
/* Debug / test hook: the geometry the direct binning (option "direct_binning", default on: tile lists by per-chunk tile histograms,
 * column scans and a one-wave-per-chunk scatter instead of emit + tile sort + ranges) would use for N Gaussians on T tiles:
 * out[0..6] = { 1 if the direct route serves this frame (0: the sort route -- more than 4 096 tiles, or N out of range),
 * Gaussians per chunk S (a multiple of 64), chunks NC, groups G, chunks per group Cg, T rounded up to 64, scratch bytes }.  Host only. */
int gsr_debug_direct_binning_geometry(int32_t N, int32_t T, int64_t out[7]);
/* The balanced placement's per-view cost caches of the CURRENT device for frames of W x H (synchronises the device):
 * out = {lookups, hits, entries in use, caches}.  A hit = the render found the entry of its frame (by GsrForwardArgs::view_id,
 * or by pose within "view_pose_tol_e6") and placed its waves by that frame's previous visit counts. */
int gsr_debug_view_cache_stats(int32_t W, int32_t H, int64_t out[4]);
/* The list cut's counters ("list_cut") of the CURRENT device for frames of W x H (synchronises the device): out = {renders that ran
 * the cut machinery, renders whose repair pass found flagged tiles, tiles repaired, chunks of the depth order behind the frame's cut
 * (summed), deep tiles (summed)}. */
int gsr_debug_list_cut_stats(int32_t W, int32_t H, int64_t out[5]);
/* Sum of the recorded durations of stage `name` ("preprocess_fwd", "sort_depth", "scan", "emit", "sort_tile",
 * "ranges", "blend_fwd", "blend_bwd", "preprocess_bwd") since the last read; synchronises on the events.  With the direct binning
 * "scan" = k_chunk_counts + the two column scans, "emit" = k_chunk_scatter, "sort_tile" / "ranges" record nothing. */
int gsr_profile_read(const char* name, double* total_ms, int64_t* count);

/* ---- "next" row f-3: fused photometric loss of the train step -----------------------
 * loss = (1-lambda)*mean|x-y| + lambda*(1-mean SSIM(x,y)), x = clamp(render,0,1) when clamp01_render != 0.
 * Replaces the torch ops of /root/reference/trainer/losses.py:98-136 (Loss.forward) and :147-209 (11x11 Gaussian
 * window SSIM) applied to the clamped render of /root/reference/scene/gaussian_model_ht.py:883.
 * out3 = {loss, mean ssim, mean l1}; workspace (gsr_loss_workspace_bytes) is kept for the backward.
 * grad_loss: device pointer to the upstream scalar gradient, or NULL for 1. */
size_t gsr_loss_workspace_bytes(int32_t C, int32_t H, int32_t W);
int gsr_loss_forward(const float* render, const float* target, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                     int32_t clamp01_render, void* workspace, float* out3, void* stream);
int gsr_loss_backward(const float* render, const float* target, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                      int32_t clamp01_render, const void* workspace, const float* grad_loss, float* d_render,
                      void* stream);

/* The same over a stack of `images` independent images [images, C, H, W] (a batched render, GsrBatch): every image is normalised by
 * its own C H W.  out3 = {SUM of the images' losses, mean SSIM, mean L1}; the backward returns the gradient of that sum, i.e. each
 * image receives exactly the gradient of its own loss. */
size_t gsr_loss_workspace_bytes_batched(int32_t images, int32_t C, int32_t H, int32_t W);
int gsr_loss_forward_batched(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                             int32_t clamp01_render, void* workspace, float* out3, void* stream);
int gsr_loss_backward_batched(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                              int32_t clamp01_render, const void* workspace, const float* grad_loss, float* d_render, void* stream);
/* gsr_loss_forward_batched with everything `Loss.forward` returns (/root/reference/trainer/losses.py:128-136) computed by the same
 * finishing kernel: out6 = {loss, mean SSIM, mean L1, loss_rgb = (1 - lambda) mean L1, loss_dssim = 1 - mean SSIM, loss_depth = 0}
 * -- the caller slices the vector instead of launching a torch kernel per term.  loss_copy (may be NULL): a second place for out6[0]
 * (the binding's differentiable scalar lives in storage of its own). */
int gsr_loss_forward_terms(const float* render, const float* target, int32_t images, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                           int32_t clamp01_render, void* workspace, float* out6, float* loss_copy, void* stream);

/* ---- "next" row f-3, depth term (version 112): `lambda_depth * get_depth_loss(depth_pred, depth_gt)` of Loss.forward ---------
 * Replaces the torch statements of /root/reference/trainer/losses.py:114-119 (the two masked clamp assignments and the call) and
 * :86-95 (get_depth_loss): kind GSR_DEPTH_LOSS_L1 = sum |pc - g| / (H W) (:88-89); GSR_DEPTH_LOSS_INVARIANT = the MiDaS
 * scale-and-shift-invariant loss as constructed at :41 (alpha = 0.5, scales = 1, batch-based reduction; :259-393) with the mask
 * depth_gt > 0.02 (:92).  pc = min(max(depth, clamp_lo), clamp_hi) is fused (the reference clamps to [0.02, 20]); a pixel strictly
 * outside the bounds gets zero gradient, one on a bound passes it.  The gradient flows through the fitted scale and shift, as under
 * autograd in the reference.  depth, depth_gt: [H,W] float32 planes on the device.
 * All sums are float64 over fixed grids in a fixed order (no atomics): the same input gives the same bits on every run.  No host
 * synchronisation (the reference has three: `det.nonzero()` :274 and `if divisor == 0` :290 twice).
 * out6 = {loss_depth (unweighted, as Loss.forward reports it, :133), scale s, shift t, M = number of valid pixels (H W for l1), data term,
 * regulariser (before its 0.5)}.  lambda_depth is recorded in the workspace next to the coefficients; the weighted term is
 * lambda_depth * out6[0].  workspace (gsr_depth_loss_workspace_bytes, 8-byte aligned) is kept for the backward.
 * gsr_depth_loss_backward: d_depth[H,W] = grad_loss * lambda_depth * d loss_depth / d depth, one store per pixel; grad_loss = device
 * pointer to the upstream scalar gradient, or NULL for 1. */
#define GSR_DEPTH_LOSS_L1 0
#define GSR_DEPTH_LOSS_INVARIANT 1
size_t gsr_depth_loss_workspace_bytes(int32_t H, int32_t W);
int gsr_depth_loss_forward(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                           float lambda_depth, void* workspace, float* out6, void* stream);
int gsr_depth_loss_backward(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                            float lambda_depth, const void* workspace, const float* grad_loss, float* d_depth, void* stream);
/* gsr_depth_loss_forward behind gsr_loss_forward_terms on the same stream: the finishing kernel completes that call's six-float vector
 * into the whole dict of Loss.forward (:123-136) -- terms6[0] += lambda_depth * loss_depth, terms6[5] = loss_depth -- and writes the
 * new total to loss_copy (may be NULL) as well. */
int gsr_depth_loss_forward_terms(const float* depth, const float* depth_gt, int32_t H, int32_t W, int32_t kind, float clamp_lo, float clamp_hi,
                                 float lambda_depth, void* workspace, float* out6, float* terms6, float* loss_copy, void* stream);

/* The same over a stack of `images` independent planes [images, H, W] (version 114; the depth output of a batched render, GsrBatch):
 * plane b lies at b H W floats, image b owns the b-th slice of the workspace (gsr_depth_loss_workspace_bytes_batched, 8-byte aligned)
 * and nothing is shared between images -- every image has its own fit (s, t), its own M and its own determinant.  Still four short
 * launches forward and one backward, whatever `images` is (the image index is a grid dimension).
 * out6 = [images, 6], row b as gsr_depth_loss_forward writes it for plane b; *out_sum = the SUM of the images' unweighted terms, added
 * in float64 in index order (no atomics).  The backward returns the gradient of that sum: d_depth[images,H,W], image b receives exactly
 * grad_loss * lambda_depth * d loss_b / d depth_b.
 * Position independence: row b and gradient plane b are, bit for bit, what the single-plane entries give on a separately allocated,
 * 16-byte aligned copy of plane b -- whatever `images` is and wherever the plane lies (planes 1, 2, 3 ... of a stack are not 16-byte
 * aligned when H W is not a multiple of 4: every lane then still adds the elements an aligned plane gives it, only the width of its
 * loads follows the address).
 * gsr_depth_loss_forward_terms_batched runs behind gsr_loss_forward_terms(..., images, ...) on the same stream and completes its
 * six-float vector as that call's finishing kernel does for a stack: terms6[0] += lambda_depth * SUM_b loss_b, terms6[5] = the MEAN over
 * the images of the unweighted term; loss_copy (may be NULL) receives the new total.
 * GSR_ERR_ARG: images <= 0 (or more than 65535), a NULL pointer, a bad kind, a workspace that is not 8-byte aligned. */
size_t gsr_depth_loss_workspace_bytes_batched(int32_t images, int32_t H, int32_t W);
int gsr_depth_loss_forward_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind, float clamp_lo,
                                   float clamp_hi, float lambda_depth, void* workspace, float* out6 /* [images,6] */, float* out_sum /* 1 float */,
                                   void* stream);
int gsr_depth_loss_backward_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind, float clamp_lo,
                                    float clamp_hi, float lambda_depth, const void* workspace, const float* grad_loss,
                                    float* d_depth /* [images,H,W] */, void* stream);
int gsr_depth_loss_forward_terms_batched(const float* depth, const float* depth_gt, int32_t images, int32_t H, int32_t W, int32_t kind,
                                         float clamp_lo, float clamp_hi, float lambda_depth, void* workspace, float* out6 /* [images,6] */,
                                         float* terms6, float* loss_copy, void* stream);

/* ---- "next" row f-2: multi-tensor Adam step in one launch ------------------------------------------------
 * Same update rule as torch.optim.Adam(l, lr=0.0, eps=1e-15) of /root/reference/scene/gaussian_model_ht.py:275-289
 * (no amsgrad, no weight decay); `step` is the 1-based step count used for the bias corrections. */
#define GSR_ADAM_MAX_TENSORS 8
typedef struct GsrAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    uint64_t n;  /* elements */
    float lr;
} GsrAdamTensor;
int gsr_adam_step(const GsrAdamTensor* tensors, int32_t count, float beta1, float beta2, float eps, int64_t step,
                  void* stream);

/* Pose step of stage A (extension f-4; compute_relative_pose, trainer/ht3dgs_trainer.py:308-333): the pose being fitted is
 * M = Exp(delta) * base with six tangent numbers delta = (tau[3], phi[3]) under Adam -- `LieGroupParameter.retr()` +
 * torch.optim.Adam in the reference.  step >= 1: chains d_points_transform12 (dL/dM, as written by gsr_backward) to dL/d(delta),
 * applies torch's Adam update (lr, beta1, beta2, eps; bias correction for `step`) to delta6 / exp_avg6 / exp_avg_sq6 in place
 * and writes the new M (3x4 row-major) to points_transform_out12 -- where the next gsr_forward reads its points_transform.
 * step = 0: only evaluates M for the current delta.  base12 = NULL: identity.  All pointers device; one one-thread kernel. */
int gsr_pose_step(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_points_transform12, const float* base12,
                  float* points_transform_out12, float lr, float beta1, float beta2, float eps, int64_t step, void* stream);
/* gsr_pose_step for P >= 1 independent poses in ONE launch (one 64-lane workgroup per pose): pose p lives at p * 6 floats of delta6 /
 * exp_avg6 / exp_avg_sq6 and p * 12 floats of d_points_transform12 (as gsr_backward_views writes it), base12 ([P,12] or NULL) and
 * points_transform_out12.  Every pose gets, bit for bit, what gsr_pose_step gives it alone, step = 0 included. */
int gsr_pose_step_many(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_points_transform12,
                       const float* base12 /* [P,12] or NULL */, float* points_transform_out12, int32_t P, float lr, float beta1, float beta2,
                       float eps, int64_t step, void* stream);

/* The chain of gsr_pose_step alone (round 6): d_delta6_out = dL/d(delta) of M = Exp(delta) * base given dL/dM
 * (d_points_transform12, as written by gsr_backward), nothing updated.  It is the backward of the autograd node that stands where the
 * unmodified trainer evaluates `P[k].retr()` (scene/gaussian_model_ht.py:135-148): `.grad` of the frame's six pose numbers is
 * left where the trainer's own optimizer object looks for it (trainer/ht3dgs_trainer.py:162-166).  base12 = NULL: identity. */
int gsr_pose_grad(const float* delta6, const float* d_points_transform12, const float* base12, float* d_delta6_out, void* stream);

/* The same step when the pose lives in the render's CAMERA (the reference's camera_optimizer stepping a frame's pose after each
 * render of it, trainer/ht3dgs_trainer.py:162-166): viewmatrix = M^T, projmatrix = viewmatrix * projection_T, campos = -R^T t for
 * the world-to-camera M = Exp(delta) * base.  Takes gsr_backward's d_viewmatrix / d_projmatrix / d_campos (any may be NULL),
 * folds them into dL/dM, chains to dL/d(delta), applies Adam and rewrites the three camera tensors IN PLACE for the next render
 * of the frame.  projection_T16 = the transposed projection of the camera's intrinsics (projmatrix = viewmatrix * projection_T).
 * step = 0: only evaluates the camera tensors for the current delta. */
int gsr_pose_step_camera(float* delta6, float* exp_avg6, float* exp_avg_sq6, const float* d_viewmatrix16, const float* d_projmatrix16,
                         const float* d_campos3, const float* projection_T16, const float* base12, float* viewmatrix16,
                         float* projmatrix16, float* campos3, float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* The trainer's per-iteration bookkeeping between backward() and optimizer.step() (trainer/ht3dgs_trainer.py:137-148), one launch
 * each instead of the reference's ~25 small torch kernels (what gsr_autopatch routes the unmodified trainer's statements to):
 *   gsr_masked_max         dst[i] = max(dst[i], (float)src[i]) where mask[i]: `max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis])`
 *   gsr_densify_stats_add  HTGaussianModel.add_densification_stats (scene/gaussian_model_ht.py:718-721): accum[i] += |grad[i, :2]|,
 *                          denom[i] += 1 where mask[i]; viewspace_grad3 = the [N,3] gradient of the screen-space points
 *   gsr_psnr               utils/image_utils.py:16-18 `psnr(img1, img2)`: out[c] = 20 log10(1 / sqrt(mean_c (a - b)^2)) for C planes of P
 *                          pixels each; scratch = gsr_psnr_scratch_bytes(C) bytes (two launches: partial sums, finish)
 * mask: one byte per element (torch.bool). */
int gsr_masked_max(float* dst, const int32_t* src, const uint8_t* mask, int32_t n, void* stream);
int gsr_densify_stats_add(float* xyz_gradient_accum, float* denom, const float* viewspace_grad3, const uint8_t* mask, int32_t n, void* stream);
size_t gsr_psnr_scratch_bytes(int32_t C);
int gsr_psnr(const float* a, const float* b, int32_t C, int64_t P, float* out, void* scratch, void* stream);

/* ---- version 117: the per-model exit decision of a launch chain (gsr_forward_retire), two launches: partial sums, finish.
 * render, target: stacks [B,C,H,W] (B = 1: one image).  mse_b = mean over the C H W elements of image b of (clamp(render, 0, 1) - target)^2;
 * every difference and square is formed in float64 from the float32 inputs and the values are added in a fixed order over a fixed grid
 * (no atomics), the element -> lane assignment depending on the position INSIDE the image alone: mse_out[b] and the decision of image b are
 * bit-identical whatever B is and wherever the image lies in the stack.  mse_out: B doubles, always written.  The finishing kernel sets
 *     retired_at[b] = step   when   retired_at[b] == 0  &&  step > exit_after  &&  mse_b < mse_bar     (strict; a NaN never retires)
 * and never changes an entry that is set (sticky).  mse_bar = 10^(-psnr_exit / 10) as a double; the reference's rule is exit_after = 500,
 * psnr_exit = 35 (/root/reference/trainer/ht3dgs_trainer.py:299-300).  scratch: gsr_batch_retire_scratch_bytes(B) bytes, 8-byte aligned.
 * GSR_ERR_ARG: a NULL pointer, B outside 1..65535, a non-positive C / H / W, step < 1 or beyond int32, exit_after < 0, mse_out or scratch
 * not 8-byte aligned. */
size_t gsr_batch_retire_scratch_bytes(int32_t B);
int gsr_batch_retire(const float* render, const float* target, int32_t B, int32_t C, int32_t H, int32_t W, double mse_bar, int64_t exit_after,
                     int64_t step, int32_t* retired_at, double* mse_out, void* scratch, void* stream);

/* ---- "next" row f-1: simple_knn._C.distCUDA2 ----------------------------------------------------------------
 * out[i] = mean of the squared distances from points[i] to its 3 nearest other points (exact), the semantics of the
 * reference's SciPy twin /root/reference/scene/gaussian_model_ht.py:31-36; called at :211-216. */
size_t gsr_knn_scratch_bytes(int32_t N);
int gsr_knn_mean_dist2(const float* points /*[N,3]*/, int32_t N, float* out /*[N]*/, void* scratch, size_t scratch_bytes,
                       void* stream);

/* ---- the single-image model's point cloud: depth map -> points -> voxel-grid means (version 118) --------------------------------------
 * The two steps the reference runs in front of create_from_pcd for every frame of stage A and every leaf, on the host
 * (/root/reference/trainer/trainer.py:646-671).  Neither kornia nor Open3D is available where this library is built and tested: both
 * entries RESTATE the libraries' public definitions, they are not pinned against a run of them.  Both calls are
 * fully asynchronous on `stream`.
 *
 * gsr_depth_to_points -- replaces `kornia.geometry.depth.depth_to_3d(depth[None,None], K[None], normalize_points=False)` at
 * /root/reference/trainer/trainer.py:646-650.  For pixel column u = 0..W-1 and row v = 0..H-1 (integer pixel coordinates as float32) and
 * d = depth[v,u]:
 *     x = ((u - cx) / fx) * d      y = ((v - cy) / fy) * d      z = d
 * all in float32 in exactly that order: a subtraction, a division, a product, each rounded once (nothing of it can contract to an FMA).
 * points: row-major [H*W,3] (row v*W + u).  image [3,H,W] and colors [H*W,3] are given BOTH or NEITHER: colors[v*W+u, c] = image[c,v,u]
 * (the reference's `image_np.reshape(-1, 3)` of the [H,W,3] image, :662; its points are reshaped the same way, :652).
 * GSR_ERR_ARG (before anything is enqueued): depth or points NULL, H or W not positive, H*W >= 2^31, fx or fy equal to 0, image without
 * colors or the reverse.
 *
 * gsr_voxel_down_sample -- replaces Open3D's `PointCloud::VoxelDownSample` (`pcd.voxel_down_sample(voxel_size=0.01)`,
 * /root/reference/trainer/trainer.py:664-665; the `estimate_normals` before it, :663, produces normals nothing reads and has no counterpart):
 *   * points and colours are widened to float64;
 *   * min_bound = the per-axis minimum over the FINITE points (all three coordinates finite), origin = min_bound - 0.5 * voxel_size;
 *   * the voxel index of a point per axis is floor((p - origin) / voxel_size) in float64;
 *   * every occupied voxel yields one output point = the mean of its points and one colour = the mean of their colours, both accumulated in
 *     float64 and rounded ONCE to float32; out_counts[m] = the number of points of voxel m;
 *   * a point with a non-finite coordinate belongs to no voxel, does not enter the bound and is counted in `dropped`;
 *   * output order: ascending (ix, iy, iz), lexicographic.  Open3D's own order is that of its hash map and unspecified; this one is defined
 *     and repeatable.
 * The sums are taken in a fixed order that depends on a voxel's point count alone (csrc/voxel_kernels.hip; no floating-point atomics): two
 * calls on the same input are bit-identical, and voxels of up to 16 points are summed in input order.
 * meta (device, 4 x int64, 8-byte aligned; the caller reads it): {M = number of voxels, dropped, status, 0}.  status = 1 when an axis needs
 * an index >= 2^21 (extent / voxel_size too large for the 63-bit key ix<<42 | iy<<21 | iz): then M = 0 and no output row is to be relied on.
 * out_points / out_colors / out_counts have room for N rows; rows [0, M) are written.  colors and out_colors are given BOTH or NEITHER;
 * out_counts may be NULL.  scratch: gsr_voxel_scratch_bytes(N) bytes, 8-byte aligned -- a closed form in N, monotone, 0 for N <= 0.
 * N == 0: returns 0, writes meta = {0,0,0,0} and launches nothing else (every other pointer may be NULL).
 * GSR_ERR_ARG (before anything is enqueued): N < 0 or N >= 2^31, meta NULL or not 8-byte aligned, voxel_size <= 0 or not finite, colors
 * without out_colors or the reverse, and for N > 0 points, out_points or scratch NULL, scratch misaligned or shorter than
 * gsr_voxel_scratch_bytes(N). */
int    gsr_depth_to_points(const float* depth /*[H,W]*/, const float* image /*[3,H,W] or NULL*/, int32_t H, int32_t W,
                           float fx, float fy, float cx, float cy, float* points /*[H*W,3]*/, float* colors /*[H*W,3] or NULL*/, void* stream);
size_t gsr_voxel_scratch_bytes(int64_t N);
int    gsr_voxel_down_sample(const float* points /*[N,3]*/, const float* colors /*[N,3] or NULL*/, int64_t N, double voxel_size,
                             float* out_points /*[N,3] capacity*/, float* out_colors /*[N,3] or NULL*/, int32_t* out_counts /*[N] or NULL*/,
                             int64_t* meta /*device, 4 x int64: M, dropped, status, 0*/, void* scratch, size_t scratch_bytes, void* stream);

/* ---- cameras from device poses (version 119) ---------------------------------------------------------------------------------------------
 * Both entries are one launch of one wave, fully asynchronous on `stream`, float64 inside with ONE rounding to float32 per output, and
 * evaluated without multiply-add contraction in the operation order written here (csrc/camera_kernels.hip), so that the same statements in
 * host float64 give the same bits wherever no sin / cos / acos is involved.  4x4 matrices are row-major float32.
 *
 * gsr_camera_from_pose -- replaces the matrices `Camera(is_co3d=True)` builds per call (/root/reference/scene/cameras.py:76-98: the
 * transpose at :78-80, the projection at :83-91, the `bmm` at :97 and the `inverse()` at :98, which waits for the device) behind
 * `load_viewpoint_cam(idx, pose)` (/root/reference/trainer/trainer.py:1098-1132).  pose[b] = world-to-camera, last row (0,0,0,1), b < B:
 *   viewmatrix[b][i][j] = pose[b][j][i]                                  (world_view_transform; a copy)
 *   P = [[2 fx / W, 0, -(W - 2 cx) / W, 0], [0, 2 fy / H, -(H - 2 cy) / H, 0], [0, 0, zfar / (zfar - znear), -(zfar znear) / (zfar - znear)],
 *        [0, 0, 1, 0]]  in float64 from the arguments as given (the reference rounds these entries to float32 first: its full projection
 *        may differ from this one in the last float32 bit)
 *   projmatrix[b][i][j] = ((pose[0][i] P[j][0] + pose[1][i] P[j][1]) + pose[2][i] P[j][2]) + pose[3][i] P[j][3]     (full_proj_transform)
 *   campos[b][i] = -(((adj[i][0] t0 + adj[i][1] t1) + adj[i][2] t2) / det),  A = pose[:3,:3], t = pose[:3,3], adj = the adjugate of A,
 *        det = (A00 adj00 + A01 adj10) + A02 adj20                        (camera_center = -A^-1 t; A need not be orthonormal)
 * GSR_ERR_ARG (before anything is enqueued): a NULL pointer, B < 1 or B > 16, W or H not positive, fx or fy not positive, a non-finite
 * intrinsic or plane, zfar == znear.
 *
 * gsr_pose_virtual_view -- replaces `get_virtual_view` (/root/reference/trainer/ht3dgs_trainer.py:462-479) and, with `base`, the
 * teacher-relative pose of :878.  Poses are taken as rigid 3x4 blocks (the last row of every output is written as (0,0,0,1)):
 *   rel = pose0^-1 pose1 (inverse by the adjugate);  phi = Log of its rotation: theta = acos(clamp((trace - 1) / 2)), phi = k w with
 *   w = the half antisymmetric part, k = theta / sin(theta), or 1 + theta^2 / 6 below theta = 1e-4;  tau = V(phi)^-1 t (adjugate);
 *   out = pose0 Exp(alpha (tau, phi)), Exp = (R, V tau') with R = I + a K + b K^2, V = I + b K + c K^2, a = sin t / t, b = (1 - cos t) / t^2,
 *   c = (t - sin t) / t^3, or their two-term series below t^2 = 1e-8 (the switches of pose.py);  out_rel = out base^-1.
 * base and out_rel are given BOTH or NEITHER.  alpha = 0 returns pose0 bit for bit.
 * GSR_ERR_ARG (before anything is enqueued): pose0, pose1 or out NULL, base without out_rel or the reverse, alpha outside [0, 1] or NaN. */
int gsr_camera_from_pose(const float* pose /*[B,16]*/, int32_t B, double fx, double fy, double cx, double cy, int32_t W, int32_t H,
                         double znear, double zfar, float* viewmatrix /*[B,16]*/, float* projmatrix /*[B,16]*/, float* campos /*[B,3]*/,
                         void* stream);
int gsr_pose_virtual_view(const float* pose0 /*[16]*/, const float* pose1 /*[16]*/, double alpha, const float* base /*[16] or NULL*/,
                          float* out /*[16]*/, float* out_rel /*[16] or NULL*/, void* stream);

/* ---- resizing the model on the device (version 120) -------------------------------------------------------------------------------------
 * Pruning and densification replace every per-Gaussian tensor (six parameter groups, twelve Adam moments) by a tensor of another length.
 * The two entries decide the new layout from one flag byte per row and move the rows.  Neither computes a float: every byte they write is
 * a copy of a byte the caller supplied, or zero.  Both are asynchronous on `stream`; no workgroup waits for another one.
 *
 * Flag bits of row i (flags: uint8 [N], device):
 *   GSR_RESIZE_KEEP   the row survives as itself, parameters and moments;
 *   GSR_RESIZE_CLONE  a copy of the row's parameters is appended with zero moments;
 *   GSR_RESIZE_SPLIT  the row is a split parent: it takes a rank among the split parents, in ascending row order;
 *   GSR_RESIZE_CHILD  (with SPLIT; ignored without it) the split parent's two children survive.
 * The new layout, nA + nB + 2 nC rows, is: A = the KEEP rows ascending; B = the CLONE rows ascending; C = the SPLIT + CHILD rows
 * ascending, copy 0; then the same rows again, copy 1 -- the order in which "append the clones, append both copies of the children, prune
 * the parents, prune" leaves them.
 *
 * gsr_resize_plan writes the plan, the scratch and meta, nothing else.
 *   plan: gsr_resize_plan_bytes(N) bytes, 4-byte aligned: GSR_RESIZE_PLAN_SEGMENTS segments of int32, each S = 64 * ceil(N / 64) entries
 *         long (segment k starts at entry k * S):
 *           GSR_RESIZE_PLAN_ROWS_A      [nA]      the KEEP rows
 *           GSR_RESIZE_PLAN_ROWS_B      [nB]      the CLONE rows
 *           GSR_RESIZE_PLAN_ROWS_C      [nC]      the SPLIT + CHILD rows
 *           GSR_RESIZE_PLAN_RANK_C      [nC]      the split rank of each of them (its position in the next list)
 *           GSR_RESIZE_PLAN_SPLIT_ROWS  [nSplit]  all SPLIT rows, with children or not (the caller gathers the parents with it)
 *         entries beyond a list's length are not written.
 *   meta: GSR_RESIZE_META_WORDS x int64 on the device, 8-byte aligned: {nA, nB, nC, nSplit, status, 0, 0, 0}.  The plan clears the status;
 *         gsr_resize_apply raises it.  The caller reads meta (its one host wait) and passes the four counts to gsr_resize_apply.
 *   scratch: gsr_resize_scratch_bytes(N) bytes, 4-byte aligned.  Both sizes are closed forms in N, monotone, 0 for N <= 0.
 *   N == 0: meta is zeroed, nothing else is touched (flags, plan and scratch may be NULL).
 *   GSR_ERR_ARG (before anything is enqueued; gsr_last_error() names the rule): N < 0 or N >= 2^31, meta NULL or misaligned, and for N > 0
 *   flags, plan or scratch NULL, plan or scratch misaligned or shorter than its size function says.
 *
 * gsr_resize_apply writes every destination row of up to GSR_RESIZE_MAX_TENSORS tensors in one launch.  Tensor k has N source rows and
 * nA + nB + 2 nC destination rows of row_bytes bytes each (a multiple of 4; rows are moved in 4-byte words); dst is a fresh buffer that
 * overlaps nothing.  By kind:
 *   GSR_RESIZE_PARAM          every destination row is the copy of its source row;
 *   GSR_RESIZE_MOMENT         the rows of A are copies, the rows of B and C are zero (all bits);
 *   GSR_RESIZE_CHILD_SOURCED  as PARAM, but copy c of the C entry with split rank r is row c * nSplit + r of `child`, a caller tensor of
 *                             2 nSplit rows (the sampled positions and the shrunken scales of the children).
 * A tensor with row_bytes == 0, or with src and dst both NULL, is skipped (a zero-width group; moments that do not exist yet).
 * Every row number read from the plan is compared with N (a rank: with nSplit) before it is used as an address; an entry that fails writes
 * its destination row as zeros and sets meta[GSR_RESIZE_META_STATUS] to 1.  A wrong plan is a status, never an access out of bounds.
 * nA + nB + 2 nC == 0 (nothing kept) and N == 0 are not errors: nothing is launched.
 * GSR_ERR_ARG (before anything is enqueued; gsr_last_error() names the rule): N < 0 or N >= 2^31, meta NULL or misaligned, count < 0 or
 * beyond GSR_RESIZE_MAX_TENSORS, tensors NULL with count > 0, a count outside the plan's capacity (0 <= nA, nB, nSplit <= N, 0 <= nC <=
 * nSplit), plan NULL, misaligned or shorter than gsr_resize_plan_bytes(N) when there are rows to write, a row_bytes that is negative, not a
 * multiple of 4 or 2^31 and more, an unknown kind, src without dst or the reverse, a misaligned src / dst / child, a CHILD_SOURCED tensor
 * without child when nC > 0. */
#define GSR_RESIZE_KEEP 1
#define GSR_RESIZE_CLONE 2
#define GSR_RESIZE_SPLIT 4
#define GSR_RESIZE_CHILD 8
#define GSR_RESIZE_PARAM 0
#define GSR_RESIZE_MOMENT 1
#define GSR_RESIZE_CHILD_SOURCED 2
#define GSR_RESIZE_MAX_TENSORS 18
#define GSR_RESIZE_META_WORDS 8
#define GSR_RESIZE_META_STATUS 4
#define GSR_RESIZE_PLAN_SEGMENTS 5
#define GSR_RESIZE_PLAN_ROWS_A 0
#define GSR_RESIZE_PLAN_ROWS_B 1
#define GSR_RESIZE_PLAN_ROWS_C 2
#define GSR_RESIZE_PLAN_RANK_C 3
#define GSR_RESIZE_PLAN_SPLIT_ROWS 4
typedef struct GsrResizeTensor {
    const void* src;      /* [N, row_bytes] */
    void* dst;            /* [nA + nB + 2 nC, row_bytes] */
    const void* child;    /* [2 nSplit, row_bytes]: GSR_RESIZE_CHILD_SOURCED only, NULL otherwise */
    int64_t row_bytes;
    int32_t kind;
    int32_t reserved;
} GsrResizeTensor;
size_t gsr_resize_scratch_bytes(int64_t N);
size_t gsr_resize_plan_bytes(int64_t N);
int    gsr_resize_plan(const uint8_t* flags /*[N]*/, int64_t N, void* plan, size_t plan_bytes, int64_t* meta /*device, 8 x int64*/,
                       void* scratch, size_t scratch_bytes, void* stream);
int    gsr_resize_apply(const void* plan, size_t plan_bytes, int64_t N, int64_t nA, int64_t nB, int64_t nC, int64_t nSplit,
                        const GsrResizeTensor* tensors, int32_t count, int64_t* meta, void* stream);

/* ---- resizing the models of a batch (version 122) ----------------------------------------------------------------------------------------
 * The same two steps over B models that share one store (GsrBatch: model b owns the 128-row blocks [first_block[b], first_block[b + 1]);
 * its own rows are the first counts[b] of them, the rest of its last block is padding).  Integers decide and bytes are copied, as above;
 * the number of launches does not depend on B, and no workgroup waits for another one.
 *
 * GsrResizeBatch (host memory): B in [1, GSR_RESIZE_MAX_MODELS], first_block[0 .. B] starting at 0 and not decreasing, counts[b] in
 * [0, 128 * (first_block[b + 1] - first_block[b])].  The store has N = 128 * first_block[B] rows, N < 2^31.
 *
 * gsr_resize_plan_batched: flags uint8 [N] as above.  Row i of model b is store row 128 * first_block[b] + i for i < counts[b]; the flag
 * byte of any other row (padding) is ignored, whatever it holds.
 *   plan: gsr_resize_plan_bytes(N) bytes: the five segments of gsr_resize_plan, S = N entries each.  Model b's four lists and its split
 *         ranks are those gsr_resize_plan gives the model alone, each ascending, and start at entry 128 * first_block[b] of their segment
 *         (a list is never longer than its model).  ROW NUMBERS ARE STORE ROWS (an index_select of the store with a SPLIT_ROWS list gathers
 *         the model's split parents); SPLIT RANKS ARE MODEL-LOCAL.  Entries beyond a list's length are not written.
 *   meta: [B][GSR_RESIZE_META_WORDS] int64 on the device, 8-byte aligned; row b = {nA_b, nB_b, nC_b, nSplit_b, status_b = 0, 0, 0, 0}.
 *   scratch: gsr_resize_scratch_bytes_batched(N) bytes, 4-byte aligned (four counters per 128-row block: a block belongs to one model,
 *         where a 256-row tile could hold the end of one and the start of the next); a closed form in N, monotone, 0 for N <= 0.
 *   N == 0 (models without blocks only): meta is zeroed, nothing else is touched.
 *   A repeat of the call is bit-identical: integer sums in a fixed order, no atomics.
 *   GSR_ERR_ARG (before anything is enqueued; gsr_last_error() names the rule): batch NULL, B outside [1, 16], a first_block that does not
 *   start at 0 or decreases, a counts[b] that is negative or beyond its model's blocks, N >= 2^31, meta NULL or misaligned, and for N > 0
 *   flags, plan or scratch NULL, plan or scratch misaligned or shorter than its size function says.
 *
 * gsr_resize_apply_batched writes every row of the new store, padding included, for up to GSR_RESIZE_MAX_TENSORS tensors in one launch.
 *   old_batch        the batch the plan was made for;  counts4 (host, [B][4]) = {nA_b, nB_b, nC_b, nSplit_b} as read from meta.
 *   new_first_block  (host, [B + 1]) starts at 0 with new_first_block[b + 1] - new_first_block[b] = max(1, ceil(n'_b / 128)), n'_b = nA_b +
 *                    nB_b + 2 nC_b: a model that loses every row keeps one block of padding, so model numbers stay what they were.  Any
 *                    other new_first_block is refused.  The new store has N' = 128 * new_first_block[B] rows; dst is [N', row_bytes].
 *   Model b's rows start at row 128 * new_first_block[b] in the single-model order (A, B, C copy 0, C copy 1); from there to the end of its
 *   last block the rows are padding.  A padding row of a PARAM or CHILD_SOURCED tensor is the tensor's `pad` row (row_bytes bytes on the
 *   device; NULL: zeros), a padding row of a MOMENT tensor is zero.  MOMENT keeps its meaning per model (A copied, B and C zero).  The
 *   `child` tensor of a CHILD_SOURCED tensor holds the models' children back to back: model b's part starts at row 2 * sum_{j<b} nSplit_j,
 *   and inside it copy c of rank r is row c * nSplit_b + r.
 *   Every row number read from the plan is compared with its model's rows [128 * first_block[b], 128 * first_block[b] + counts[b]) before
 *   it is used as an address, a rank with nSplit_b; an entry that fails writes its destination row as zeros and sets
 *   meta[b][GSR_RESIZE_META_STATUS] to 1.  A wrong plan is a status in its model's row, never an access out of bounds.
 *   GSR_ERR_ARG (before anything is enqueued): the rules of old_batch above, counts4 or new_first_block NULL, a count beyond its model's
 *   capacity (0 <= nA_b, nB_b, nSplit_b <= counts[b], 0 <= nC_b <= nSplit_b), a new_first_block that is not exactly the one above, N' >=
 *   2^31, meta NULL or misaligned, plan NULL, misaligned or shorter than gsr_resize_plan_bytes(N) when a model keeps a row, and per tensor
 *   the row_bytes, kind, src / dst and alignment rules of gsr_resize_apply (pad is 4-byte aligned too; a CHILD_SOURCED tensor needs child
 *   when any nC_b > 0). */
#define GSR_RESIZE_MAX_MODELS 16
#define GSR_RESIZE_BLOCK 128
typedef struct GsrResizeBatch {
    int32_t B;
    int32_t reserved;
    int64_t first_block[GSR_RESIZE_MAX_MODELS + 1];
    int64_t counts[GSR_RESIZE_MAX_MODELS];
} GsrResizeBatch;
typedef struct GsrResizeBatchTensor {
    const void* src;      /* [N, row_bytes] */
    void* dst;            /* [N', row_bytes] */
    const void* child;    /* [2 sum nSplit_b, row_bytes]: GSR_RESIZE_CHILD_SOURCED only, NULL otherwise */
    const void* pad;      /* [row_bytes]: the padding row of a PARAM / CHILD_SOURCED tensor; NULL = zeros */
    int64_t row_bytes;
    int32_t kind;
    int32_t reserved;
} GsrResizeBatchTensor;
size_t gsr_resize_scratch_bytes_batched(int64_t N);
int    gsr_resize_plan_batched(const uint8_t* flags /*[N]*/, const GsrResizeBatch* batch, void* plan, size_t plan_bytes,
                               int64_t* meta /*device, [B][8] int64*/, void* scratch, size_t scratch_bytes, void* stream);
int    gsr_resize_apply_batched(const void* plan, size_t plan_bytes, const GsrResizeBatch* old_batch, const int64_t* counts4 /*host [B][4]*/,
                                const int64_t* new_first_block /*host [B+1]*/, const GsrResizeBatchTensor* tensors, int32_t count,
                                int64_t* meta /*device, [B][8] int64*/, void* stream);

/* ---- the merge on the device (version 121) -----------------------------------------------------------------------------------------------
 * merge_two_3DGS drops the prune_ratio * N Gaussians of least importance on both sides and appends what is left of the source to what is
 * left of the destination.  Two entries: which rows go (gsr_select_smallest), and the move of two models' kept rows into one (gsr_merge_apply,
 * after one gsr_resize_plan per model).  Like the resize they decide with integers and copy bytes; both are asynchronous on `stream`, wait
 * for nothing on the host, and no workgroup waits for another one.
 *
 * gsr_select_smallest: the k rows of values [N, C] (float32, row-major, device) with the smallest row maximum.
 *   score  the maximum of the row's C values; a NaN anywhere in the row makes the score NaN (torch.amax).
 *   key    the score as an unsigned 32-bit integer that orders like the float: -0 counts as +0; a non-negative float is its bits with the
 *          sign bit set, a negative one the complement of its bits (so negatives order below positives and -inf is lowest); every NaN is
 *          0xffffffff, the largest key of all -- the order of torch.topk(largest=False).
 *   The k rows with the smallest keys are selected.  AMONG ROWS WHOSE KEY EQUALS THE k-TH SMALLEST KEY (the threshold key), THOSE WITH THE
 *   LOWEST ROW NUMBERS ARE TAKEN: the selection is np.argsort(key, kind="stable")[:k], where torch.topk promises no rule.
 *   drop        [N] or NULL: 1 for a selected row, 0 otherwise (a torch bool mask, byte for byte).
 *   keep_flags  [N] or NULL: GSR_RESIZE_KEEP for a row that is not selected, 0 for a selected one: the flag bytes gsr_resize_plan takes.
 *   meta        GSR_SELECT_META_WORDS x int64 on the device, 8-byte aligned: {k, rows with a key below the threshold key, rows with the
 *               threshold key, the threshold key, NaN rows, status = 0, 0, 0}.  With k == 0 nothing is selected and the threshold key and
 *               the two counts beside it are 0 (the NaN rows are still counted); with N == 0 all eight words are 0.
 *   scratch     gsr_select_scratch_bytes(N) bytes, 4-byte aligned (the keys, four histograms of 256 bins, one counter per 256 rows): a
 *               closed form in N, monotone, 0 for N <= 0.
 *   The only float operations are comparisons.  Histograms are summed with integer atomics, whose result does not depend on their order: a
 *   repeat of the call is bit-identical.  Addresses are formed from row numbers below N, tile numbers below ceil(N / 256) and digits below
 *   256 only; the positions counted by the histograms are compared with k and with each other, never added to a pointer.
 *   GSR_SELECT_MAX_COLUMNS is 64: with C a multiple of 4 a workgroup stages 256 rows x C / 4 partial keys in LDS, 16 KiB at the cap; 48
 *   (SH degree 3, three channels) and 64 (the same with a fourth channel) pass.  Wider inputs are reduced by the caller first.
 *   GSR_ERR_ARG (before a device is touched; gsr_last_error() names the rule): N < 0 or N >= 2^31 (a plan's row numbers are int32), C < 1
 *   or C > GSR_SELECT_MAX_COLUMNS, k < 0 or k > N, meta NULL or misaligned, and for N > 0 drop and keep_flags both NULL, values or scratch
 *   NULL or not 4-byte aligned, scratch shorter than gsr_select_scratch_bytes(N).  N == 0 (only meta is written; the other pointers
 *   may be NULL, as an empty allocation's are), k == 0 and k == N are served.
 *
 * gsr_merge_apply: plan_a / plan_b are the plans gsr_resize_plan wrote for the flag bytes of model a (Na rows) and model b (Nb rows); only
 * their GSR_RESIZE_PLAN_ROWS_A segments are read, nA / nB are the lengths the caller read from the two metas.  Destination rows [0, nA) are
 * model a's kept rows ascending, rows [nA, nA + nB) model b's: prune_points on both, then densification_postfix.  One launch over up to
 * GSR_RESIZE_MAX_TENSORS tensors, rows moved in 4-byte words; dst [nA + nB, row_bytes] is a fresh buffer that overlaps nothing.  By kind:
 *   GSR_RESIZE_PARAM   both parts are copies of their source rows;
 *   GSR_RESIZE_MOMENT  the rows of a are copies, the rows of b are zero (all bits) and src_b is not read (it may be NULL): what
 *                      cat_tensors_to_optimizer leaves of the destination's optimizer state.
 * A tensor with row_bytes == 0, or with src_a, src_b and dst all NULL, is skipped.  A plan entry outside [0, Na) (for b: [0, Nb)) is never
 * used as an address: its destination row is written as zeros and meta[GSR_RESIZE_META_STATUS] is set to 1 (meta: 8 x int64 on the
 * device, either plan's meta -- gsr_resize_plan cleared its status word).  nA + nB == 0 is not an error: nothing is launched.
 * GSR_ERR_ARG (before anything is enqueued): Na or Nb outside [0, 2^31), meta NULL or misaligned, count < 0 or beyond
 * GSR_RESIZE_MAX_TENSORS, tensors NULL with count > 0, nA outside [0, Na] or nB outside [0, Nb], plan_a (plan_b) NULL, misaligned or
 * shorter than gsr_resize_plan_bytes(Na) (Nb) when nA > 0 (nB > 0), a row_bytes that is negative, not a multiple of 4 or 2^31 and more, a
 * kind other than PARAM and MOMENT, sources without dst, src_a NULL with nA > 0, src_b NULL on a PARAM tensor with nB > 0, a misaligned
 * src_a / src_b / dst. */
#define GSR_SELECT_MAX_COLUMNS 64
#define GSR_SELECT_META_WORDS 8
typedef struct GsrMergeTensor {
    const void* src_a;    /* [Na, row_bytes] */
    const void* src_b;    /* [Nb, row_bytes]; may be NULL for GSR_RESIZE_MOMENT */
    void* dst;            /* [nA + nB, row_bytes] */
    int64_t row_bytes;
    int32_t kind;
    int32_t reserved;
} GsrMergeTensor;
size_t gsr_select_scratch_bytes(int64_t N);
int    gsr_select_smallest(const float* values /*[N,C] row-major*/, int64_t N, int32_t C, int64_t k, uint8_t* drop /*[N] or NULL*/,
                           uint8_t* keep_flags /*[N] or NULL*/, int64_t* meta /*device, 8 x int64*/, void* scratch, size_t scratch_bytes,
                           void* stream);
int    gsr_merge_apply(const void* plan_a, size_t plan_a_bytes, int64_t Na, int64_t nA, const void* plan_b, size_t plan_b_bytes, int64_t Nb,
                       int64_t nB, const GsrMergeTensor* tensors, int32_t count, int64_t* meta, void* stream);

/* Measurement hook (bench.py roofline.peak_measured): float4 streaming copy of `bytes` bytes (a multiple of 16, 16-byte aligned
 * pointers) with `blocks` workgroups of 256 threads.  variant 0 = plain loads / stores, 1 = nt bit, 2 = four loads in flight per
 * lane (nt), 3 = persistent workgroups (a few hundred), contiguous runs, eight loads in flight per lane (nt).  The best achieved read +
 * write rate is the practical HBM ceiling of the box for a streaming kernel. */
int gsr_stream_copy(const void* src, void* dst, size_t bytes, int variant, int blocks, void* stream);

/* Building blocks exported for the unit tests of tests/test_gpu_blocks.py (device pointers): stable sort of (key, value) pairs on key
 * bits [begin_bit, end_bit), 0 <= begin_bit < end_bit <= width of the key (anything else: GSR_ERR_ARG); the result is in the _alt
 * buffers when *result_in_alt comes back 1.  gsr_knn_mean_dist2 sorts its Morton keys through gsr_sort_pairs_u32. */
int gsr_sort_pairs_u32(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, uint32_t n,
                       int begin_bit, int end_bit, void* scratch, size_t scratch_bytes, int* result_in_alt,
                       void* stream);
int gsr_sort_pairs_u16(uint16_t* keys, uint32_t* vals, uint16_t* keys_alt, uint32_t* vals_alt, uint32_t n,
                       int begin_bit, int end_bit, void* scratch, size_t scratch_bytes, int* result_in_alt,
                       void* stream);
size_t gsr_sort_scratch_bytes(uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
