/*
 * topo4d_raster.h — C ABI of the MI355X-native differentiable Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary for the ONE hot path of Topo4D: the rasterizer behind
 *     im, radius, depth, alpha = Renderer(raster_settings=cam)(**rendervar)
 * (/root/reference train.py:307, :388, :463, :484; imports train.py:19, helpers.py:18-19).
 * Upstream binds that path through a pybind11 module `diff_gaussian_rasterization._C` with the entry points
 * `rasterize_gaussians`, `rasterize_gaussians_backward` and `mark_visible` (not vendored in the reference —
 * README.md:22-24).  The functions below are what a maintainer binds instead (ctypes stub in
 * INTEGRATION.md; the shipped Python host side is topo4d_amd/rasterizer.py):
 *
 *   t4d_rasterize_forward   <->  _C.rasterize_gaussians            (called from train.py:307/388/463/484)
 *   t4d_rasterize_backward  <->  _C.rasterize_gaussians_backward   (reached from loss.backward(), train.py:667/738)
 *   t4d_mark_visible        <->  _C.mark_visible                   (GaussianRasterizer.markVisible; unused by Topo4D)
 *   t4d_state_bytes / t4d_backward_scratch_bytes  <->  upstream's resize-callback buffers (geom/binning/img)
 *
 * Conventions
 *   - plain C: raw DEVICE pointers (fp32 unless noted), sizes, and a hipStream_t passed as void*.
 *     No torch types.  The library never allocates or frees device memory and never synchronises the
 *     stream unless T4D_FLAG_CHECKED / T4D_FLAG_DEBUG_SYNC asks for it.
 *   - one call renders n_views views of the SAME P Gaussians (the 24 cameras of a Topo4D frame, or one rank's
 *     shard of them); n_views = 1 is the reference's call shape.  All views share H and W.
 *     (T4DProblem.views_per_param_set lets one call carry the views of SEVERAL frames, each frame with its own P Gaussians.)
 *   - per-view camera record = T4D_VIEW_FLOATS floats on the device, built from the fields of
 *     GaussianRasterizationSettings (helpers.py:73-86):
 *        [0..15]  viewmatrix  — the 16 floats of the [1,4,4] tensor helpers.py:67 builds (transposed w2c ⇒
 *                 element (row r, col c) of the mathematical matrix sits at [c*4+r])
 *        [16..31] projmatrix  — same layout (helpers.py:71-72)
 *        [32..34] campos      [35..37] bg      [38] tanfovx      [39] tanfovy
 *   - outputs are planar, one image after another: color [V,3,H,W], depth [V,1,H,W], alpha [V,1,H,W],
 *     radii int32 [V,P] — for V = 1 exactly the four tensors train.py:307 unpacks.
 *   - gradients are per view: dL_dX has a leading V dimension; the caller sums over views if it wants the
 *     gradient of a multi-view loss (or passes T4D_FLAG_... none: summation is not done here).
 *   - every function returns T4D_OK (0) or an error code; nothing throws or exits across the ABI.
 */
#ifndef TOPO4D_RASTER_H
#define TOPO4D_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T4D_ABI_VERSION 4
#define T4D_VIEW_FLOATS 40
#define T4D_GRAD_PAIR_FLOATS 10   /* per (Gaussian,tile) partial-gradient record in the backward scratch */

enum {
    T4D_OK = 0,
    T4D_ERR_ARG = 1,            /* bad argument combination (mirrors the upstream Python-level checks) */
    T4D_ERR_HIP = 2,            /* a HIP runtime call failed; see t4d_last_error() */
    T4D_ERR_PAIR_OVERFLOW = 3,  /* pair_capacity too small (CHECKED mode): status->max_pairs_per_view says how much */
    T4D_ERR_STATE_SIZE = 4      /* state/scratch buffer smaller than t4d_*_bytes() */
};

enum {
    T4D_FLAG_CHECKED = 1u,     /* forward: sync once after binning sizes are known and fail with PAIR_OVERFLOW
                                  instead of rendering truncated tile lists (what upstream's num_rendered D2H does) */
    T4D_FLAG_DEBUG_SYNC = 2u,  /* `debug=True` of the settings tuple: synchronise + check after every kernel */
    T4D_FLAG_PREFILTERED = 4u, /* accepted for API parity (helpers.py:84 passes False); no effect */
    T4D_FLAG_ASYNC_STATUS = 8u,/* forward, without CHECKED: `status` must point at PINNED (device-mapped) host memory; the first
                                  16 bytes receive { uint32 overflow; uint32 max_pairs_per_view; uint64 total_pairs } without
                                  any host synchronisation: written by the binning kernel itself (one view of at most 1,024
                                  tiles; the two 8-byte words may land one after the other) or by an asynchronous copy
                                  enqueued behind the binning kernels */
    T4D_FLAG_NO_LONG_BINS = 16u,/* forward: the caller knows (T4DStatus.max_tile_pairs of an earlier call on this scene) that no
                                  tile list exceeds 2048 pairs: the launch of the long-bin sort kernel is skipped, and a one-view
                                  launch of more than 8,192 tiles keeps no snapshots for a depth-segmented backward of its long
                                  tiles.  Only a speed hint — longer bins that show up anyway are still sorted and replayed
                                  correctly, just slowly */
    T4D_FLAG_SHORT_BINS = 32u, /* forward: ... and that none exceeds 512 pairs (the one-pass ranking sort): a small launch then
                                  sorts every bin inside the render workgroup of its tile instead of launching a sort kernel.
                                  A speed hint like the one above */
    T4D_FLAG_LONG_LISTS = 64u, /* forward: the caller knows that some tile list exceeds 1,024 pairs: launches of up to 24 x CUs
                                  tiles (instead of 12 x) run the latency build of the forward, which such a list bounds.
                                  A speed hint */
    T4D_FLAG_RAW_PARAMS = 128u /* forward AND backward of a call: `rotations`, `opacities`, `scales` are Topo4D's optimiser
                                  parameters - un-normalised quaternions, logit opacities, log scales (helpers.py:95-97) - the
                                  library applies F.normalize / sigmoid / exp itself (the arithmetic of t4d_activate_forward), and
                                  the backward returns dL/d(unnorm_rotations), dL/d(logit_opacities), dL/d(log_scales) in
                                  dL_drotations, dL_dopacities, dL_dscales (per view; the arithmetic of t4d_activate_backward):
                                  params2rendervar and its autograd without a launch of their own */
};

typedef struct T4DProblem {
    int32_t abi_version;     /* = T4D_ABI_VERSION */
    int32_t n_views;         /* V */
    int32_t P;               /* Gaussians */
    int32_t H, W;            /* image_height, image_width */
    int32_t sh_degree;       /* active SH degree (settings.sh_degree); used only when shs != NULL */
    int32_t sh_coeffs;       /* M: coefficients stored per Gaussian in shs [P,M,3] */
    float   scale_modifier;
    int64_t pair_capacity;   /* capacity, PER VIEW, of the (Gaussian,tile) pair arena */
    uint32_t flags;
    uint32_t views_per_param_set; /* 0 (or n_views): every view renders the same P Gaussians - one frame per call.
                                     k > 0: the call carries n_views / k PARAMETER SETS (frames) of P Gaussians each, view v renders
                                     set v / k; every per-Gaussian INPUT array (means3D, opacities, scales, rotations,
                                     cov3D_precomp, colors_precomp, shs) then holds the sets one after the other, [n_views / k][P, .].
                                     n_views must be a multiple of k.  Outputs and gradients keep their per-view layout ([V, ...]),
                                     so nothing else changes: a rank of a view-sharded job (BASELINE config 3: 3 of 24 cameras per
                                     rank) renders its cameras of several independent frames in ONE launch set, at the efficiency
                                     of a 24-view launch.  Results per view are those of the same view in a one-frame call of the
                                     same launch shape */
} T4DProblem;

typedef struct T4DStatus {
    int64_t max_pairs_per_view;  /* largest per-view number of (Gaussian,tile) pairs this call needed */
    int64_t total_pairs;         /* sum over views (upstream's num_rendered, summed) */
    int32_t overflow;            /* 1 if any view exceeded pair_capacity (its tile lists were truncated) */
    int32_t max_tile_pairs;      /* longest per-tile list of the call (dense passes reach > 10^4; see T4D_FLAG_NO_LONG_BINS) */
} T4DStatus;

typedef struct T4DForwardIO {
    const float *views;           /* [V][T4D_VIEW_FLOATS] */
    const float *means3D;         /* [P,3] */
    const float *opacities;       /* [P] (the [P,1] tensor of helpers.py:96) */
    const float *scales;          /* [P,3] or NULL when cov3D_precomp */
    const float *rotations;       /* [P,4] (r,x,y,z), caller-normalised (helpers.py:95), or NULL */
    const float *cov3D_precomp;   /* [P,6] or NULL */
    const float *colors_precomp;  /* [P,3] or NULL when shs */
    const float *shs;             /* [P,M,3] or NULL */
    float   *out_color;           /* [V,3,H,W] */
    float   *out_depth;           /* [V,1,H,W] */
    float   *out_alpha;           /* [V,1,H,W] */
    int32_t *out_radii;           /* [V,P] */
    void    *state;               /* opaque, t4d_state_bytes(); must stay alive and unmodified until backward */
    size_t   state_bytes;
} T4DForwardIO;

typedef struct T4DBackwardIO {
    const float *views, *means3D, *opacities, *scales, *rotations, *cov3D_precomp, *colors_precomp, *shs;
    const int32_t *radii;         /* the [V,P] forward output */
    const void  *state;           /* the forward's state buffer */
    size_t       state_bytes;
    const float *dL_dcolor;       /* [V,3,H,W] */
    const float *dL_ddepth;       /* [V,1,H,W] or NULL (= zeros; Topo4D discards depth, train.py:307) */
    const float *dL_dalpha;       /* [V,1,H,W] or NULL */
    float *dL_dmeans3D;           /* [V,P,3] */
    float *dL_dmeans2D;           /* [V,P,3] (z = 0): the screen-space gradient kept alive by train.py:304 */
    float *dL_dcolors;            /* [V,P,3]   or NULL (required when colors_precomp) */
    float *dL_dshs;               /* [V,P,M,3] or NULL (required when shs) */
    float *dL_dopacities;         /* [V,P] */
    float *dL_dscales;            /* [V,P,3]   or NULL (required unless cov3D_precomp) */
    float *dL_drotations;         /* [V,P,4]   or NULL (required unless cov3D_precomp) */
    float *dL_dcov3D;             /* [V,P,6]   or NULL (required when cov3D_precomp) */
    void  *scratch;               /* t4d_backward_scratch_bytes() */
    size_t scratch_bytes;
    float *cotangent_dot;         /* [V] or NULL.  out[v] = <color, dL_dcolor> + <depth, dL_ddepth> + <alpha, dL_dalpha> of view v:
                                   * the replay's suffix sum IS this inner product when it reaches the eye, so the backward
                                   * emits it for one reduction per tile instead of a second pass over both images
                                   * (deterministic; agrees with the sum over the forward's outputs to fp32 rounding) */
} T4DBackwardIO;

uint32_t    t4d_abi_version(void);
const char *t4d_last_error(void);

size_t t4d_state_bytes(const T4DProblem *prob);
size_t t4d_backward_scratch_bytes(const T4DProblem *prob);

/* Forward: preprocess -> per-tile binning -> per-tile depth sort -> alpha blend.  `status` may be NULL; it is
 * filled only in CHECKED / DEBUG_SYNC mode (otherwise use t4d_fetch_status after the stream has drained). */
int t4d_rasterize_forward(const T4DProblem *prob, const T4DForwardIO *io, T4DStatus *status, void *hip_stream);

/* Backward: per-tile back-to-front replay (atomic-free, deterministic) -> per-Gaussian gather + chain rule.
 * If the forward that produced `state` overflowed its pair arena (only possible without T4D_FLAG_CHECKED), every
 * gradient of this call is written as ZERO: a truncated pass never yields garbage.
 * `prob` must be the T4DProblem of the forward that produced `state`, FLAGS INCLUDED: which kernels run (whole tiles or depth
 * segments, one launch or two) is re-derived from it, not read from the state.  The mix that goes wrong: a forward with
 * T4D_FLAG_NO_LONG_BINS on a one-view launch of more than 8,192 tiles keeps no slot table, and a backward of the same call without
 * the flag leaves the long tiles out of its whole-tile launch, expecting segments that were never written. */
int t4d_rasterize_backward(const T4DProblem *prob, const T4DBackwardIO *io, void *hip_stream);

/* Copies the status block of a forward's state buffer to the host (synchronises the stream). */
int t4d_fetch_status(const T4DProblem *prob, const void *state, T4DStatus *out, void *hip_stream);

/* present[i] = 1 iff Gaussian i passes the near-plane test of view record `view` (upstream markVisible). */
int t4d_mark_visible(int32_t P, const float *means3D, const float *view, uint8_t *present, void *hip_stream);

/* out[v] = sum_i a[v][i] * b[v][i] for v < n_views (one fused pass, deterministic): per-view scalars for a multi-GPU loss
 * gather.  (For sum(colour * dL/dcolour) itself, T4DBackwardIO.cotangent_dot is free; bench.py uses that.) */
size_t t4d_view_dot_scratch_bytes(int32_t n_views);
int t4d_view_dot(int32_t n_views, int64_t n_per_view, const float *a, const float *b, float *out, void *scratch,
                 void *hip_stream);

/* The gradient of a loss that ADDS per-view terms (rasterize_views: one launch set per frame, one optimiser step per frame):
 * dst[k][i] = sum over v < n_views of src[k][v * n_per_view[k] + i], v ascending (deterministic), for up to T4D_SUM_MAX_TENSORS
 * per-view gradient tensors of t4d_rasterize_backward in ONE launch (six torch reductions otherwise).  NULL entries are skipped. */
#define T4D_SUM_MAX_TENSORS 8
int t4d_sum_views(int32_t n_views, int32_t n_tensors, const float *const *src, float *const *dst, const int64_t *n_per_view,
                  void *hip_stream);

/* Fused photometric loss of Topo4D's render loop, forward AND gradient in one call (train.py:310,315;
 * helpers.py:115-116 l1_loss_v1; external.py:73-116 calc_ssim):
 *     im' = exp(cam_m[v,c]) * im + cam_c[v,c];   loss[v] = 0.8*mean|im'-gt| + 0.2*(1 - mean SSIM_11x11(im', gt))
 * im, gt, dL_dim: [V,3,H,W]; cam_m, cam_c, dL_dcam_m, dL_dcam_c: [V,3] (both NULL = no affine / no gradient wanted);
 * view_weight [V] = dL/dloss[v] (NULL = 1).  dL_dim is exactly the dL_dcolor input of t4d_rasterize_backward. */
size_t t4d_photometric_scratch_bytes(int32_t n_views, int32_t H, int32_t W);
int t4d_photometric_loss(int32_t n_views, int32_t H, int32_t W, const float *im, const float *gt, const float *cam_m,
                         const float *cam_c, const float *view_weight, float *loss, float *dL_dim, float *dL_dcam_m,
                         float *dL_dcam_c, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Masked L1 of the dense (texture) pass, train.py:394-405 (get_loss_dense with use_mask=True): no camera affine, no SSIM,
 *     loss[v] = sum over { mask == 1 } of |im - gt|  /  count{ mask == 1 },     dL_dim = view_weight[v] * sign(im - gt) / count there, 0 elsewhere.
 * im, gt, mask, dL_dim: [V,3,H,W]; mask is the float image of zeros and ones helpers.get_mask (helpers.py:811-823) returns
 * (the three channels carry the same plane; they are all counted, like `masked_index.sum()`).  An empty mask gives NaN, as
 * in the reference. */
size_t t4d_masked_l1_scratch_bytes(int32_t n_views);
int t4d_masked_l1_loss(int32_t n_views, int32_t H, int32_t W, const float *im, const float *gt, const float *mask,
                       const float *view_weight, float *loss, float *dL_dim, void *scratch, size_t scratch_bytes, void *hip_stream);

/* helpers.get_mask (helpers.py:811-823) and the masked target of get_loss's later-frame branch (train.py:320-326; train.py:631,647
 * hard-code use_mask = True, so this is what every frame after the first optimises against), for the n_views cameras of a
 * frame in ONE launch - the reference recomputes both in every iteration although they depend on (frame, camera) only.
 *     hit(pixel)    = OR over the n_labels selected labels of  AND over channels c of  | mask_image[c]*255 - label_colors[k][c] | < 1
 *     filtered_mask = 1 where hit else 0, on all three channels           (get_mask's return value; NULL = not wanted)
 *     target        = gt * scale where hit else gt                         (masked_gt, scale = 0.1 at train.py:326; NULL = not wanted)
 * mask_image, gt, filtered_mask, target: [V,3,H,W] device floats; mask_image is the label image as get_dataset loads it
 * (train.py:84-92: 8-bit colours / 255).  label_colors: HOST array [n_labels,3] of the selected labels' colours as floats, in the
 * channel order of the mask image (helpers.py:806 `cmap`: the pascal colormap of 14 labels with its columns swapped to BGR),
 * n_labels <= T4D_MAX_MASK_LABELS.  Arithmetic is the reference's, rounding for rounding (float32 product, then float32
 * difference): filtered_mask and target are bit-identical to torch's. */
#define T4D_MAX_MASK_LABELS 16
int t4d_label_mask_target(int32_t n_views, int32_t H, int32_t W, const float *mask_image, const float *label_colors /* host */,
                          int32_t n_labels, const float *gt, float scale, float *filtered_mask, float *target, void *hip_stream);

/* The 'soft_color' term of get_loss_dense (train.py:407; weight 0.02, train.py:541-543): helpers.l1_loss_v2 (helpers.py:119-120)
 *     *loss = mean over rows of ( sum over width of |x - y| )                                   (UNWEIGHTED, device scalar)
 *     grad[i] (+)= (weight / rows) * sign(x[i] - y[i])     (sign(0) = 0 as torch's abs; accumulate != 0: added to what grad holds -
 *                                                           e.g. t4d_rasterize_backward's dL_dcolors; grad NULL = no gradient)
 * x = dense_rgb_colors, y = dense_init_colors: [rows,width] device floats.  Deterministic (fixed partial-sum order). */
size_t t4d_soft_color_scratch_bytes(void);
int t4d_soft_color_loss(int64_t rows, int32_t width, const float *x, const float *y, float weight, float *loss, float *grad,
                        int32_t accumulate, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Topology priors of the geometry loop: the regularisers of get_loss (train.py:328-368) on the RAW parameters, forward and
 * backward in two launches, no host synchronisation, no floating-point atomics (bit-identical from run to run).
 *   later frames (is_initial == 0): rigid, rot, iso (train.py:330-346); flat, flat_lip_bottom (FlattenLoss); flat_eye,
 *     flat_face_bottom, flat_lip_socket (FlattenLoss_v2); flat_lid_top, flat_lid_bottom, flat_lip, flat_mouth (SoftFlattenLoss
 *     against cos_init) (train.py:349-357)
 *   frame 0 (is_initial != 0): scale, scale_max, and the four soft terms without cos_init, whose cos is written into cos_init
 *     (train.py:359-368)
 * means3D [P,3], unnorm_rotations [P,4], log_scales [P,3]: the optimiser's tensors (normalize / exp of helpers.py:91-100 are
 * applied inside).  losses [T4D_PRIORS_TERMS + 1]: weights[t] * L_t in the T4D_PRIOR_* order (0 for the terms the frame does not
 * evaluate), then their sum.  d_* (+)= upstream * dL/d(raw tensor) (upstream NULL: 1; flags & T4D_PRIORS_ACCUMULATE: added to what
 * the buffers hold, e.g. t4d_rasterize_backward's gradients; otherwise overwritten).  Every index array is validated by the caller
 * (0 <= index < P): the kernels do not check them. */
#define T4D_PRIORS_TERMS 14
enum { T4D_PRIOR_SCALE, T4D_PRIOR_SCALE_MAX, T4D_PRIOR_RIGID, T4D_PRIOR_ROT, T4D_PRIOR_ISO, T4D_PRIOR_FLAT,
       T4D_PRIOR_FLAT_LIP_BOTTOM, T4D_PRIOR_FLAT_EYE, T4D_PRIOR_FLAT_FACE_BOTTOM, T4D_PRIOR_FLAT_LIP_SOCKET,
       T4D_PRIOR_FLAT_LID_TOP, T4D_PRIOR_FLAT_LID_BOTTOM, T4D_PRIOR_FLAT_LIP, T4D_PRIOR_FLAT_MOUTH };
#define T4D_PRIORS_EDGE_TERMS 6     /* flat, flat_lip_bottom, flat_lid_top, flat_lid_bottom, flat_lip, flat_mouth */
#define T4D_PRIORS_REGION_TERMS 3   /* flat_eye, flat_face_bottom, flat_lip_socket */
#define T4D_PRIORS_ACCUMULATE 1
typedef struct T4DPriors {
    int32_t P, K;                               /* Gaussians (= mesh vertices), padded one-ring width */
    const int32_t *nbr;                         /* [P,K] neighbor_indices, padded with the vertex's own index */
    const float *nbr_dist, *rig_w, *rot_w, *iso_w, *nbr_mask;   /* [P,K]; nbr_mask: FlattenLoss_v2's 0/1 padding mask */
    const int32_t *nbr_num;                     /* [P] one-ring sizes (FlattenLoss_v2.neighbor_num) */
    const float *init_scale;                    /* [P] */
    int32_t n_edges[T4D_PRIORS_EDGE_TERMS];     /* interior edges of each flatten term, in the order above */
    const int32_t *edges[T4D_PRIORS_EDGE_TERMS];/* [4, n]: v0s | v1s | v2s | v3s */
    int32_t n_region[T4D_PRIORS_REGION_TERMS];
    const int32_t *region[T4D_PRIORS_REGION_TERMS];
    /* transposed incidence (CSR, built once by the caller): nbr_t_idx[nbr_t_off[v] .. nbr_t_off[v+1]) = every e = g*K+k with
     * nbr[e] == v, ascending; rec_idx[f][rec_off[f][v] .. ) = the position records (t4d_priors_record_layout) that name vertex v
     * among the terms frame kind f evaluates (f = 0: frame 0, 1: later frames), ascending */
    const int32_t *nbr_t_off, *nbr_t_idx;
    const int32_t *rec_off[2], *rec_idx[2];
    float weights[T4D_PRIORS_TERMS];            /* losses_weights (train.py:535-540) */
    /* per-frame state (initialize_per_timestep, train.py:420-438; cos_init: train.py:365-368) */
    const float *prev_inv_rot;                  /* [P,4] */
    const float *prev_offset;                   /* [P,K,3] */
    float *cos_init[4];                         /* flat_lid_top, flat_lid_bottom, flat_lip, flat_mouth: [n_edges] */
} T4DPriors;
/* Position records: edge term t occupies 4 * n_edges[t] records (record base + 4 i + j names vertex edges[t][j * n + i]), region
 * term r occupies (K + 1) * n_region[r] (slot k < K names nbr[v, k], slot K the region vertex v itself), in the order edge terms
 * 0..5 then region terms 0..2.  Returns the total number of records and writes each term's first record into base[9]. */
int64_t t4d_priors_record_layout(const T4DPriors *pr, int64_t *base);
size_t t4d_priors_scratch_bytes(const T4DPriors *pr);
int t4d_priors_eval(const T4DPriors *pr, int32_t is_initial, const float *means3D, const float *unnorm_rotations,
                    const float *log_scales, float *d_means3D, float *d_unnorm_rotations, float *d_log_scales,
                    const float *upstream, uint32_t flags, float *losses, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Fused optimiser step of Topo4D's loop: torch.optim.Adam (one group per tensor, train.py:272-297) for up to
 * T4D_ADAM_MAX_TENSORS tensors in ONE launch, followed by the per-iteration region freezes of train.py:676-700
 * (`params[name][mask] = values`) expressed as a per-row pin mask + pinned values.  grad == NULL: the tensor only gets its
 * pins (torch skips parameters without a gradient). */
#define T4D_ADAM_MAX_TENSORS 12
typedef struct T4DAdamTensor {
    float *param;               /* [rows, width] updated in place (rows == 0: a no-op, may be NULL) */
    const float *grad;          /* same shape or NULL */
    float *exp_avg, *exp_avg_sq;/* Adam state, same shape (required when grad != NULL) */
    const uint8_t *pin_mask;    /* [rows] or NULL */
    const float *pin_values;    /* [rows, width] (read where pin_mask != 0) or NULL */
    int64_t rows;
    int32_t width;
    float lr;
    int32_t step;               /* 1-based count of the gradient steps THIS tensor has taken, this one included (torch keeps
                                   the step per parameter; a tensor skipped for lack of a gradient does not advance) */
    int32_t flags;              /* T4D_ADAM_CLEAR_GRAD: the step leaves zeros in `grad` (a persistent gradient buffer that the next
                                   iteration fills only in part - the per-camera rows of cam_m / cam_c, train.py:310 - needs no
                                   separate fill launch); 0 otherwise */
} T4DAdamTensor;
#define T4D_ADAM_CLEAR_GRAD 1
int t4d_adam_pin_step(const T4DAdamTensor *tensors /* host array */, int32_t n_tensors, float beta1, float beta2, float eps,
                      void *hip_stream);
/* The same step with its hyper-parameters in DEVICE memory, so that the launch can be recorded in a HIP graph and replayed - ONE
 * launch: lr_dev [n_tensors] float learning rates; step_dev [t4d_adam_step_counters(tensors, n)] int32 step counts, one PER WORKGROUP
 * of the launch (workgroups of 256 elements, tensor after tensor in descriptor order: tensor k owns ceil(rows_k * width_k / 256)
 * consecutive counters, all equal - read any of them).  A workgroup of a tensor that has a gradient advances its own counter, then
 * uses it for the bias corrections (a tensor skipped for lack of a gradient does not advance).  The `step` and `lr` fields of the
 * descriptors are ignored.  Bias corrections are evaluated in double precision on the device: results equal t4d_adam_pin_step's.
 * The descriptors' shapes must be the same in every call that shares a step_dev array: n_step_counters - the length of step_dev -
 * is checked against t4d_adam_step_counters(tensors, n_tensors) (T4D_ERR_ARG otherwise; nothing is launched). */
int64_t t4d_adam_step_counters(const T4DAdamTensor *tensors /* host array */, int32_t n_tensors);
int t4d_adam_pin_step_graph(const T4DAdamTensor *tensors /* host array */, int32_t n_tensors, float beta1, float beta2, float eps,
                            int32_t *step_dev, int64_t n_step_counters, const float *lr_dev, void *hip_stream);

/* Dense-attribute interpolation: helpers.py:237-253 `compute_vertex_attribute_by_weight_2` on the device (Topo4D runs it in
 * numpy after a device->host copy every frame, train.py:504-506).  out [n_coarse+n_dense, width]: the first n_coarse rows
 * copy `attribute` [n_coarse, width]; dense row d = sum_k attribute[quad_faces[vertex_father[d]][k]] * weight[d][k], k < 4,
 * accumulated in float64 like numpy and rounded to float32 once (bit-identical to the reference followed by `.float()`). */
int t4d_dense_interpolate(const float *attribute, const int32_t *quad_faces /* [n_quads,4] */,
                          const int32_t *vertex_father /* [n_dense] */, const double *weight /* [n_dense,4] */,
                          int64_t n_coarse, int64_t n_dense, int32_t width, float *out, void *hip_stream);

/* UV-space densification of the texture pass: train.py:214-243 - helpers.build_dense_vertices_2 / bilinear_interpolate_2
 * (helpers.py:421-654), the face lists of train.py:233-236 and triangulate_faces (helpers.py:657-667) - on the device, in the same
 * order and with the same bits (the reference runs it once per run in Python: minutes at --density 30).  The sequential `edge_dict`
 * of the reference is replaced by a host pre-pass (topo4d_amd/densify.py:plan_dense_mesh) that gives every frontal quad q:
 *   plan[2q]   = flags: bit s set = edge slot s is borrowed (slot 0: row i = 0, face[0] -> face[3]; 1: column j = 0, face[0] ->
 *                face[1]; 2: row i = d+1, face[1] -> face[2]; 3: column j = d+1, face[3] -> face[2])
 *   plan[2q+1] = the exclusive prefix sum of the quads' generated-point counts (d+2)^2 - 4 - d * popcount(flags)
 *   src[4q+s]  = owner quad * 4 + owner slot of a borrowed slot (the first frontal quad containing the edge), -1 otherwise.
 * Outputs (device): dense_vertex [n_vert + n_points, 3] float64 (float32 values: coarse rows, then the generated points),
 * vertex_father [n_points] int32, vertex_weight [n_points, 4] float64, dense_uvs [n_uv + n_points, 2] float64, and the
 * triangulated faces / uv_faces [n_faces, 3] int32: triangles, then the densified quads, then the non-frontal quads, each quad as
 * [0,1,2], [0,2,3].  Every index the kernels read is range-checked; a violation sets the int32 at the start of the scratch to a
 * nonzero value (the caller reads it after the stream) and skips the read. */
typedef struct T4DDenseMesh {
    int32_t n_vert, n_uv;                       /* coarse vertices (params['means3D'] rows), len(uvs_ori) */
    int32_t n_quads, density;                   /* frontal quads (densified), d >= 1 */
    int32_t n_tri, n_rest;                      /* triangles, non-frontal quads */
    int64_t n_points, n_faces;                  /* generated points (sum of the counts), n_tri + 2 (n_quads (d+1)^2 + n_rest) */
    const float *vertices;                      /* [n_vert,3] */
    const double *uvs;                          /* [n_uv,2] uvs_ori */
    const int32_t *quads, *uv_quads;            /* [n_quads,4] frontal quads and their UV faces, in processing order */
    const int32_t *plan, *src;                  /* [n_quads,2], [n_quads,4]: see above */
    const int32_t *tri, *uv_tri;                /* [n_tri,3] */
    const int32_t *rest, *uv_rest;              /* [n_rest,4] */
    double *dense_vertex;
    int32_t *vertex_father;
    double *vertex_weight;
    double *dense_uvs;
    int32_t *faces, *uv_faces;
} T4DDenseMesh;
size_t t4d_dense_scratch_bytes(const T4DDenseMesh *mesh);
int t4d_dense_build(const T4DDenseMesh *mesh, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Exact k-nearest-neighbour mean squared distance: helpers.py:147-157 `o3d_knn(pts, k)` followed by `.mean(-1)` (train.py:131-132
 * with k = 1, :245-246 with k = 4).  points [n,3] float64 (device); mean [n] float64: per point the k+1 smallest squared distances,
 * its own zero included, summed in ascending order and divided by k, each distance ((dx*dx + dy*dy) + dz*dz) without contraction
 * (nanoflann's L2 adaptor for dim 3) - equal to the reference's drop-the-first-hit mean whatever order ties and duplicates fall
 * in, and bit-identical from run to run.  log_scales [n,3] float32 or NULL: float(log(sqrt(max(mean, 1e-7)))) tiled to three
 * columns (dense_log_scales, train.py:262).  A hashed uniform grid over the occupied cells, searched in cube shells; no host
 * synchronisation.  1 <= k <= T4D_KNN_MAX_K, k < n < 2^30. */
#define T4D_KNN_MAX_K 15
size_t t4d_knn_scratch_bytes(int64_t n, int32_t k);
int t4d_knn_mean_sq_dist(const double *points, int64_t n, int32_t k, double *mean, float *log_scales, void *scratch,
                         size_t scratch_bytes, void *hip_stream);

/* Parameter activations of params2rendervar (helpers.py:91-100: rotations = F.normalize(unnorm_rotations), opacities =
 * sigmoid(logit_opacities), scales = exp(log_scales)) in one launch, and their vector-Jacobian products in one launch
 * (torch runs three kernels forward and about a dozen through autograd backward, every iteration: SURVEY.md row a2).
 * All pointers are device pointers; rotations [P,4], opacities [P,1], scales [P,3].  In the backward a NULL cotangent
 * counts as zeros and a NULL output is skipped; `opacities` / `scales` are the forward OUTPUTS. */
int t4d_activate_forward(int64_t P, const float *unnorm_rotations, const float *logit_opacities, const float *log_scales,
                         float *rotations, float *opacities, float *scales, void *hip_stream);
int t4d_activate_backward(int64_t P, const float *unnorm_rotations, const float *opacities, const float *scales,
                          const float *dL_drotations, const float *dL_dopacities, const float *dL_dscales,
                          float *dL_dunnorm_rotations, float *dL_dlogit_opacities, float *dL_dlog_scales, void *hip_stream);

/* UV-space texture bake (BASELINE config 5): drop-in for the reference's CPU rasterizer
 *     void _render_colors_core(float* image, float* vertices, int* triangles, float* colors, float* depth_buffer,
 *                              int nver, int ntri, int h, int w, int c)        face3d/mesh/cython/mesh_core.h:63-69
 * reached from helpers.py:953-960 (write_texture) via face3d/mesh/render.py:52-86 (render_colors).  Same argument
 * meaning (all pointers are DEVICE pointers here): vertices [nver,3] in pixel space (x, y, depth), triangles [ntri,3]
 * int32, colors [nver,c], image [h,w,c] in/out (zeros or a background), depth_buffer [h,w] in/out (the caller fills it
 * with -999999 like render.py:72).  Results are bit-identical to the reference, including its border-ring dilation
 * (mesh_core.cpp:211) and "first triangle wins on equal depth".  rows [row_begin,row_end) select a horizontal band of
 * the image (multi-GPU: one band per rank); pass 0,h for everything.  pair_capacity bounds the (triangle, 32x32 tile)
 * pairs; on T4D_ERR_PAIR_OVERFLOW *pairs_needed (host) holds the size to retry with.  Synchronises the stream once. */
size_t t4d_texture_bake_scratch_bytes(int32_t h, int32_t w, int64_t pair_capacity);
int t4d_texture_bake(const float *vertices, const int32_t *triangles, const float *colors, int32_t nver, int32_t ntri,
                     int32_t h, int32_t w, int32_t c, int32_t row_begin, int32_t row_end, float *image, float *depth_buffer,
                     void *scratch, size_t scratch_bytes, int64_t pair_capacity, int64_t *pairs_needed, void *hip_stream);

/* The reference's `render_colors(vertices, triangles, colors, h, w, c, BG)` as ONE call (face3d/mesh/render.py:52-86: image =
 * BG or zeros, depth_buffer = -999999, then _render_colors_core): `image` and `depth_buffer` are pure OUTPUTS here - every
 * texel of rows [row_begin,row_end) is written, winner or background (`background` [h,w,c] or NULL = zeros) - so the caller
 * fills nothing and the kernel reads no depth buffer (8192^2: 1.07 GB of fills and 0.27 GB of reads less than
 * t4d_texture_bake).  Same results bit for bit, same scratch (t4d_texture_bake_scratch_bytes) and overflow protocol. */
int t4d_texture_render_colors(const float *vertices, const int32_t *triangles, const float *colors, const float *background,
                              int32_t nver, int32_t ntri, int32_t h, int32_t w, int32_t c, int32_t row_begin, int32_t row_end,
                              float *image, float *depth_buffer, void *scratch, size_t scratch_bytes, int64_t pair_capacity,
                              int64_t *pairs_needed, void *hip_stream);

/* Texture finishing (topo4d_amd/texfinish.py, csrc/t4d_texfinish.hip): a gutter round the UV islands of a baked texture and
 * smaller levels that ignore the black background.  Every pointer is device memory; images are uint8 [h,w,c], c in {1, 3, 4};
 * a coverage is uint8 [h,w], non-zero = covered, and every coverage written holds 0 or 1; 1 <= h, w <= 65536.  Inputs and outputs
 * are separate buffers.  Arguments are checked before anything touches a device; none of these synchronises the stream.  All
 * arithmetic after the quantisation is integer, so the results do not depend on the launch shape.
 *
 * t4d_texture_coverage: coverage = depth > -999999.0f for the depth buffer float32 [h,w] of t4d_texture_render_colors /
 * t4d_texture_bake, which leave exactly -999999 where no triangle wrote (mesh_core.cpp:216).  A texel of the image's outermost
 * two-texel ring that the reference writes by extrapolation (mesh_core.cpp:211) has a depth and so counts as covered.
 * t4d_texture_quantize: float32 [h,w,c] -> uint8 by the rule of t4d_png_encode's float path: numpy's (x*255).astype(np.uint8) on
 * x86-64 (truncation toward zero to int32, low byte kept, NaN -> 0).
 * t4d_texture_erode: `rounds` (0..4) rounds; in each, a texel stays covered only if it and its 4-neighbours inside the image are
 * covered (neighbours outside the image count as covered).  0 rounds normalise the coverage to 0 / 1.
 * t4d_texture_pad: covered texels are copied through.  An uncovered texel (x, y) takes the value of the covered texel (x', y')
 * with (x-x')^2 + (y-y')^2 <= radius^2 (a disc; radius 0..64) that has the lexicographically smallest (d^2, y', x'), and its output
 * coverage is 1; with no such texel it keeps its input value and its output coverage is 0.  radius 0 is a copy.  Scratch:
 * t4d_texture_pad_scratch_bytes(h, w) (0 and a message for a bad shape); T4D_ERR_STATE_SIZE when it is smaller.
 * t4d_texture_halve: h and w even (T4D_ERR_ARG otherwise); outputs [h/2,w/2,c] and [h/2,w/2].  For each 2x2 block cnt = its covered
 * texels and, per channel, s = the sum over them: the output is (2 s + cnt) / (2 cnt) in integer arithmetic (round half up), 0 when
 * cnt = 0; the output coverage is cnt > 0.  Uncovered texels never enter an average. */
int t4d_texture_coverage(const float *depth, int32_t h, int32_t w, uint8_t *coverage, void *hip_stream);
int t4d_texture_quantize(const float *image, int32_t h, int32_t w, int32_t c, uint8_t *out, void *hip_stream);
int t4d_texture_erode(const uint8_t *coverage, int32_t h, int32_t w, int32_t rounds, uint8_t *out, void *hip_stream);
size_t t4d_texture_pad_scratch_bytes(int32_t h, int32_t w);
int t4d_texture_pad(const uint8_t *image, const uint8_t *coverage, int32_t h, int32_t w, int32_t c, int32_t radius,
                    uint8_t *out_image, uint8_t *out_coverage, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_texture_halve(const uint8_t *image, const uint8_t *coverage, int32_t h, int32_t w, int32_t c, uint8_t *out_image,
                      uint8_t *out_coverage, void *hip_stream);

/* Hole filling by push-pull (texfinish.fill, csrc/t4d_texfill.hip), of the same family and under the same conventions: the texels
 * of a projected texture that no camera saw take a smooth interpolation of the texels round them.  image uint8 [h,w,c]; valid
 * uint8 [h,w], non-zero = the texel has a colour; domain uint8 [h,w], non-zero = the texel wants a colour, NULL = every texel;
 * out_image [h,w,c]; out_filled uint8 [h,w], holding 0 or 1.  Pyramid colours are integers in units of 1/256 of an 8-bit step.
 * Level 0: C0 = 256 image where valid, V0 = valid != 0.
 * Pull: level k+1 has the size ceil(h_k / 2) x ceil(w_k / 2); for each 2x2 block (children outside the level do not exist) n = its
 * valid children and s = the sum of their colours per channel: V = n > 0 and C = (2 s + n) / (2 n) in integer division
 * (t4d_texture_halve's round half up).  Levels continue until the level is 1x1.
 * No valid texel at all: out_image = image and out_filled = 0.
 * Push, from the level below the top down to level 0: a texel (x, y) with V = 0 takes
 * (9 P[py][px] + 3 P[py][nx] + 3 P[ny][px] + P[ny][nx] + 8) >> 4 of the completed level above, P, where px = x >> 1, py = y >> 1,
 * nx = px + 1 for odd x and px - 1 for even x, ny likewise, both clamped to P's bounds; a texel with V = 1 keeps its pulled colour.
 * Output: a texel in the domain and not valid gets (C0 + 128) >> 8 and out_filled = 1; every other texel is copied through with
 * out_filled = 0.  A filled value lies between the smallest and the largest valid value of its channel.
 * Scratch: t4d_texture_fill_scratch_bytes(h, w, c) (0 and a message for a bad shape); T4D_ERR_STATE_SIZE when it is smaller. */
size_t t4d_texture_fill_scratch_bytes(int32_t h, int32_t w, int32_t c);
int t4d_texture_fill(const uint8_t *image, const uint8_t *valid, const uint8_t *domain, int32_t h, int32_t w, int32_t c,
                     uint8_t *out_image, uint8_t *out_filled, void *scratch, size_t scratch_bytes, void *hip_stream);
/* The same fill for 16-bit samples (texfinish.fill16: a quantised displacement map).  image and out_image are int32 [h,w,c]; a
 * sample is the low 16 bits of its word, 0..65535, and every output word holds 0..65535.  The rule is t4d_texture_fill's word for
 * word: C0 = 256 image, the same pull, push and output expressions.  The push sum reaches 16 * 65535 * 256 + 8, which is above 2^31
 * and below 2^32: it is taken in unsigned 32-bit arithmetic.  Scratch: t4d_texture_fill16_scratch_bytes(h, w, c), aligned to 4
 * bytes; errors as t4d_texture_fill. */
size_t t4d_texture_fill16_scratch_bytes(int32_t h, int32_t w, int32_t c);
int t4d_texture_fill16(const int32_t *image, const uint8_t *valid, const uint8_t *domain, int32_t h, int32_t w, int32_t c,
                       int32_t *out_image, uint8_t *out_filled, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Tracking drift between two frames' UV textures: a census block matcher (topo4d_amd/drift.py, csrc/t4d_drift.hip), under the
 * conventions of the texture family above.  luma_a, luma_b uint8 [h,w] (drift.luma: (77 R + 150 G + 29 B + 128) >> 8); valid_a,
 * valid_b uint8 [h,w], non-zero = the texel holds a photograph; labels uint8 [h,w], 0 = no island, one layout for both frames;
 * block B even in 8..64, stride S in 1..B, radius R in 0..16, min_count in 1..B^2; out int32 [nby,nbx,16].  Everything is integer
 * arithmetic, so the table is a pure function of the inputs; tests/drift_ref.py restates the rule in numpy.
 * Census: for texel p the 48 neighbours p + (j, i), j (rows) and i (columns) in -3..3 in row-major order without the centre; the
 * k-th sets bit k of the 64-bit word C(p) when L(neighbour) < L(p).  p is census-valid in a frame when all 49 texels lie inside the
 * image and are valid in that frame and labels[p] != 0; otherwise C(p) is unused.
 * Blocks: block (by, bx) covers rows by S .. by S + B - 1 and columns bx S .. bx S + B - 1; only blocks wholly inside the image
 * exist: nby = (h - B) / S + 1 and nbx = (w - B) / S + 1 in integer division, none when h < B or w < B (T4D_OK, nothing launched).
 * Cost: for each d = (dy, dx) in [-R, R]^2, n(d) counts the block's texels p with p census-valid in a, p + d inside the image and
 * census-valid in b, and labels[p] == labels[p + d]; c(d) is the sum over them of popcount(Ca(p) ^ Cb(p + d)).  d is admissible
 * when n(d) >= min_count.
 * Order: d1 is better than d2 when c1 n2 < c2 n1 (64-bit integers: the smaller c / n); ties go to the smaller dy^2 + dx^2, then the
 * smaller dy, then the smaller dx.  The best is the first admissible d of that order; the second is the first admissible d whose
 * Chebyshev distance max(|dy - dy_best|, |dx - dx_best|) from the best exceeds 1.
 * Output per block: dy, dx, then (c, n) of the best, of (dy - 1, dx), of (dy + 1, dx), of (dy, dx - 1), of (dy, dx + 1) and of the
 * second, then two zeros.  (0, 0) stands for a neighbour outside [-R, R]^2 or inadmissible and for a second that does not exist;
 * a block without an admissible d is all zeros.
 * Scratch: t4d_drift_scratch_bytes(h, w, block, stride, radius) (0 and a message for a bad shape or option; the census words of
 * both frames); T4D_ERR_STATE_SIZE when it is smaller.  The scratch must be aligned to 8 bytes. */
size_t t4d_drift_scratch_bytes(int32_t h, int32_t w, int32_t block, int32_t stride, int32_t radius);
int t4d_drift_match(const uint8_t *luma_a, const uint8_t *valid_a, const uint8_t *luma_b, const uint8_t *valid_b, const uint8_t *labels,
                    int32_t h, int32_t w, int32_t block, int32_t stride, int32_t radius, int32_t min_count, int32_t *out, void *scratch,
                    size_t scratch_bytes, void *hip_stream);

/* What follows from the measured drift (drift.dense_flow, drift.warp, csrc/t4d_stabilise.hip): the flow of every texel of the
 * full-resolution texture, and frame b's texture resampled through it, so that a feature sits on the texel it has in frame a.
 * Integer arithmetic in a fixed order, so both are pure functions of their inputs; tests/stabilise_ref.py restates the rule in numpy.
 * The matcher ran at level L: on maps of h x w texels, halved L times from the full resolution H x W with H = h 2^L and W = w 2^L
 * (L in 0..8; both divisible by 2^L).  A displacement d = (dy, dx) of block (by, bx), in texels of level L, says that the feature
 * at x in frame a lies at x + d in frame b.  labels uint8 [H,W] is the full-resolution island map, 0 = no island.
 * Nodes: block (by, bx) of the nby x nbx blocks of t4d_drift_match on h x w (block B, stride S) is a node at the doubled
 * full-resolution texel indices ny = 2^(L+1) (by S + B/2) - 1 and nx = 2^(L+1) (bx S + B/2) - 1: the block's centre, which falls
 * between two texels (texel y has the doubled index 2 y).  Its value is q = rint(d 2^L 256) (round half to even), int32, in units of
 * 1/256 of a full-resolution texel, with |q| <= 2^22; nodes is int32 [nby,nbx,2] = (q_y, q_x).  Its label is
 * labels[2^L (by S + B/2)][2^L (bx S + B/2)].  It takes part when kept[by][bx] (uint8 [nby,nbx]) is non-zero and its label is not 0.
 * t4d_drift_dense: with T = reach 2 S 2^L (reach in 1..4; T <= 46340, so that a weight fits 32 bits: T4D_ERR_ARG otherwise), a
 * texel (y, x) of label l != 0 gives every participating node of label l the weight wy wx, wy = max(0, T - |2 y - ny|) and wx = max(0, T - |2 x - nx|): with reach 1 the bilinear weights between the four
 * nodes round the texel, renormalised over those that take part.  num = sum of w q (per component) and den = sum of w in 64-bit
 * integers, which the bounds above keep below 2^63.  flow int32 [H,W,2] = (f_y, f_x) = floor((2 num + den) / (2 den)) and support
 * uint8 [H,W] = 1 where den > 0; a texel with l = 0 or den = 0 gets f = 0 and support = 0, and so does every texel of a shape
 * without a block (nodes and kept may then be NULL).  flow must be aligned to 8 bytes.
 * t4d_drift_warp: image uint8 [H,W,c], c in (1, 3, 4), valid uint8 [H,W] (non-zero = the texel holds a photograph) and labels are
 * frame b's; flow as above.  For texel (y, x): Y = 256 y + f_y, X = 256 x + f_x, y0 = Y >> 8, ty = Y & 255 (arithmetic shift: the
 * floor), x0 and tx likewise.  The taps (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1) weigh (256 - ty) (256 - tx),
 * (256 - ty) tx, ty (256 - tx), ty tx.  A tap is admissible when it lies inside the image, valid is non-zero there, its label equals
 * labels[y][x] and that label is not 0.  With Wt = the sum of the admissible weights, out_image = floor((2 sum of w v + Wt) / (2 Wt))
 * per channel and out_valid = 1; where Wt = 0 both are 0.  A texel without support has f = 0 and is a copy.  The outputs must not
 * be the inputs and must be aligned to 4 bytes. */
int t4d_drift_dense(const int32_t *nodes, const uint8_t *kept, const uint8_t *labels, int32_t h, int32_t w, int32_t block, int32_t stride,
                    int32_t level, int32_t reach, int32_t *flow, uint8_t *support, void *hip_stream);
int t4d_drift_warp(const uint8_t *image, const uint8_t *valid, const uint8_t *labels, const int32_t *flow, int32_t h, int32_t w, int32_t c,
                   uint8_t *out_image, uint8_t *out_valid, void *hip_stream);

/* A sequence's stabilised textures fused over time (topo4d_amd/seqtex.py, csrc/t4d_seqtex.hip): after t4d_drift_warp one texel shows
 * the same point of skin in every frame, so its samples over the frames are a time series.  Integer arithmetic, so both results are
 * pure functions of their inputs; tests/seqtex_ref.py restates the rule in numpy.
 * t4d_seqtex_select: images and valids are host arrays of n_frames device pointers (as photos of t4d_projtex_consistency), 1 <=
 * n_frames <= T4D_SEQTEX_MAX_FRAMES; images[t] uint8 [h,w,c], c in (1, 3, 4); valids[t] uint8 [h,w], non-zero = the texel holds a
 * photograph; 0 <= num <= den, 1 <= den <= 64.  Per texel, S is the set of frames whose validity is non-zero there and n = |S|:
 * out_count uint8 [h,w] = n.  With n = 0 every channel of out_image uint8 [h,w,c] is 0; otherwise k = ((n - 1) num) / den in integer
 * division and out_image[ch] is the value of rank k (0-based, ascending) among the n samples images[t][texel][ch], t in S.  (num, den)
 * = (1, 2) is the lower median, (0, 1) the minimum, (1, 1) the maximum.  With c = 4 alpha is a channel like the others.  The rank is
 * taken per channel, so the result need not be any one frame's colour.  What lies under an invalid texel is never read into a
 * result.  The same pointer may appear more than once in images or valids, and an input may have any alignment.
 * t4d_seqtex_complete: one frame against the sequence.  image uint8 [h,w,c] and valid uint8 [h,w] are the frame's, base uint8 [h,w,c]
 * and count uint8 [h,w] t4d_seqtex_select's; min_count and min_votes in 1..64, tol in 0..255 (255 never rejects).  Per texel, with
 * v = valid != 0 and n = count: outlier = v and n >= min_votes and max over the channels of |image[ch] - base[ch]| > tol.  If v and
 * not outlier, out_image = image and out_source = 1; else if n >= min_count, out_image = base and out_source = 2 where the frame had
 * nothing (v = 0), 3 where its sample was rejected; else out_image = 0 and out_source = 0.
 * Both: the outputs must not be inputs and must be aligned to 4 bytes; T4D_ERR_ARG with a message, before anything touches a
 * device, for a NULL buffer or table entry, a size or option outside the bounds above, a misaligned output or an output that is an
 * input.  Neither synchronises the stream. */
#define T4D_SEQTEX_MAX_FRAMES 64
int t4d_seqtex_select(const uint8_t *const *images, const uint8_t *const *valids, int32_t n_frames, int32_t h, int32_t w, int32_t c,
                      int32_t num, int32_t den, uint8_t *out_image, uint8_t *out_count, void *hip_stream);
int t4d_seqtex_complete(const uint8_t *image, const uint8_t *valid, const uint8_t *base, const uint8_t *count, int32_t h, int32_t w,
                        int32_t c, int32_t min_count, int32_t min_votes, int32_t tol, uint8_t *out_image, uint8_t *out_source,
                        void *hip_stream);

/* Lossless PNG encoder for a device image (write_texture(..., encoder="gpu"): the last CPU step of save_mesh, helpers.py:953-960).
 * image [h,w,c] on the device, uint8 (is_float32 = 0) or float32 (is_float32 = 1, quantised exactly like numpy's
 * (x*255).astype(np.uint8) on x86-64: truncation toward zero to int32, low byte kept, NaN -> 0); c in {1, 3, 4} gives colour
 * type 0 / 2 / 6, 8-bit, no interlace.  Writes the whole file (signature, IHDR, IDATs, IEND) to `out` (device,
 * out_capacity >= t4d_png_max_bytes) and its length to *out_bytes (device).  The rows are filtered with the PNG filter of least
 * sum |int8 residual|; the deflate stream is independent 16 KiB segments of literals and distance-1 runs under one dynamic
 * Huffman block each (or stored).  The bytes are a pure function of the pixels and the shape.  t4d_png_max_bytes is a function
 * of (h, w, c) alone, so the caller allocates once.  Does not synchronise the stream. */
size_t t4d_png_max_bytes(int32_t h, int32_t w, int32_t c);
size_t t4d_png_scratch_bytes(int32_t h, int32_t w, int32_t c);
int t4d_png_encode(const void *image, int32_t is_float32, int32_t h, int32_t w, int32_t c, uint8_t *out, size_t out_capacity,
                   int64_t *out_bytes /* device */, void *scratch, size_t scratch_bytes, void *hip_stream);
/* The same encoder for a render as torchvision's save_image writes it (train.py's progress snapshots, topo4d_amd/progress.py):
 * image [3,h,w] float32 on the device, contiguous, channel-planar; the file is RGB (colour type 2).  Each value is quantised as
 * x.mul(255).add_(0.5).clamp_(0, 255).to("cpu", torch.uint8): y = x*255 rounded to float32, then y + 0.5 rounded to float32 as a
 * separate rounding (never one fused multiply-add), then clamped to [0, 255] with NaN kept, then truncated toward zero to uint8
 * with NaN -> 0 (ATen's x86-64 conversion).  Output, out_capacity, scratch and error codes as t4d_png_encode with c = 3
 * (t4d_png_max_bytes(h, w, 3), t4d_png_scratch_bytes(h, w, 3)); arguments are checked before anything touches a device.  Does not
 * synchronise the stream. */
int t4d_png_encode_chw(const float *image, int32_t h, int32_t w, uint8_t *out, size_t out_capacity, int64_t *out_bytes /* device */,
                       void *scratch, size_t scratch_bytes, void *hip_stream);
/* The same encoder for 16-bit samples (png.encode_png16: a displacement map, its normal map).  image int32 [h,w,c] on the device,
 * c in {1, 3, 4}; a sample is the low 16 bits of its word.  IHDR carries bit depth 16 and colour type 0 / 2 / 6; a sample is
 * written high byte first, so a filtered row is 1 + 2 w c bytes, and the five filters run at a byte distance of bpp = 2 c.  The
 * filter choice (least sum |int8 residual|, the lowest filter number on a tie), the 16 KiB segments, the per-segment Huffman block,
 * CRC-32 and Adler-32 are t4d_png_encode's.  out_capacity >= t4d_png_max_bytes16(h, w, c), scratch >=
 * t4d_png_scratch_bytes16(h, w, c); error codes as t4d_png_encode.  Does not synchronise the stream. */
size_t t4d_png_max_bytes16(int32_t h, int32_t w, int32_t c);
size_t t4d_png_scratch_bytes16(int32_t h, int32_t w, int32_t c);
int t4d_png_encode16(const int32_t *image, int32_t h, int32_t w, int32_t c, uint8_t *out, size_t out_capacity,
                     int64_t *out_bytes /* device */, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Finishing a baked displacement map (topo4d_amd/dispmap.py, csrc/t4d_dispmap.hip), under the conventions of the texture family
 * above: 1 <= h, w <= 65536, device pointers, arguments checked before anything touches a device, no synchronisation.  A code map is
 * int32 [h,w] whose low 16 bits count; every output word holds 0..65535.  has uint8 [h,w], non-zero = the texel has a value;
 * labels uint8 [h,w], the texel's UV island, 0 = none.  Float64 arithmetic is done in the order written, without contraction, with
 * dot3(u, v) = (u0 v0 + u1 v1) + u2 v2 and rint rounding half to even; tests/dispmap_ref.py restates every rule in numpy.
 *
 * t4d_disp_quantize: disp float32 [h,w] (scanbake's map, scan units), hit uint8 [h,w], dist finite and > 0 (the bake's reach).
 * Where hit != 0 and disp is finite: code = 32768 + clamp(rint((double(disp) / dist) * 32767.0), -32767, 32767) and has = 1;
 * elsewhere code = 32768 and has = 0.  So 32768 is zero displacement and one code step is unit = dist / 32767 scan units.
 *
 * t4d_disp_smooth: `rounds` (0..8) rounds of a 5x5 binomial filter that stays inside an island; each round reads the output of the
 * round before.  With w = (1, 4, 6, 4, 1), a texel with has != 0 and label L != 0 takes S = sum w_j w_i code[y+j][x+i] and
 * Wt = sum w_j w_i over the taps (j, i in -2..2) that lie inside the image, have has != 0 and carry label L, and becomes
 * (2 S + Wt) / (2 Wt) in integer division; the centre always counts, so Wt >= 36.  Every other texel is copied through; has and
 * labels do not change; 0 rounds is a copy.  out must not be code.  Scratch: t4d_disp_smooth_scratch_bytes(h, w) (one more code
 * map for the rounds to alternate on), aligned to 4 bytes; T4D_ERR_STATE_SIZE when it is smaller.
 *
 * t4d_disp_normals: the tangent-space normal map of the displaced surface, normal int32 [h,w,3].  pos float32 [h,w,3] is the point
 * of the undisplaced surface per texel (projtex.surface_maps), unit finite and > 0 the scan units per code step.  For a texel with
 * has != 0 and label L != 0: xp = x + 1 if that texel is inside the image, has a value and carries label L, else x; xm, yp, ym
 * likewise.  If xp == xm, sx = 0; otherwise Tx = double(pos[y][xp]) - double(pos[y][xm]) per component, a = sqrt(dot3(Tx, Tx)),
 * sx = (double(code[y][xp] - code[y][xm]) * unit) / a, and sx = 0 when a == 0.  sy likewise along y.  Image y runs against v
 * (texture.process_uv flips it), so with +u right and +v up (the OpenGL convention) n = (-sx, +sy, 1), len = sqrt((sx sx + sy sy) +
 * 1.0), and each component is stored as clamp(rint(((n_i / len) * 0.5 + 0.5) * 65535.0), 0, 65535) (a NaN gives 0).  A texel
 * without a value or label gets the same on (0, 0, 1): (32768, 32768, 65535).  Known limit: the slopes are taken along u and v
 * separately through the surface's own texel lengths; the shear between dp/du and dp/dv and the curvature terms are ignored. */
int t4d_disp_quantize(const float *disp, const uint8_t *hit, int32_t h, int32_t w, double dist, int32_t *code, uint8_t *has,
                      void *hip_stream);
size_t t4d_disp_smooth_scratch_bytes(int32_t h, int32_t w);
int t4d_disp_smooth(const int32_t *code, const uint8_t *has, const uint8_t *labels, int32_t h, int32_t w, int32_t rounds, int32_t *out,
                    void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_disp_normals(const int32_t *code, const uint8_t *has, const uint8_t *labels, const float *pos, int32_t h, int32_t w,
                     double unit, int32_t *normal, void *hip_stream);

/* Applying a finished displacement map: the flat level-N tessellation of a triangle mesh and its displacement by the code map
 * (topo4d_amd/tessellate.py, csrc/t4d_tessellate.hip).  Device pointers, arguments checked before anything touches a device, no
 * synchronisation; float64 in the order written, without contraction, dot3 as above; tests/tessellate_ref.py restates every rule in
 * numpy.  level N is the number of segments per edge, 1 <= N <= 64, and N^2 n_tri < 2^31.
 *
 * Topology.  tri int32 [n_tri,3] holds the corners (a, b, c) of every triangle, a, b, c distinct and in [0, n_corner); the n_edges
 * undirected edges are the sorted pairs (lo < hi) in lexicographic order; tri_edge int32 [n_tri,3] names the edge of (a, b), (b, c)
 * and (c, a); edges int32 [n_edges,3] holds (lo, hi, owner): the owner is the lowest triangle that has the edge.  With
 * I = (N - 1)(N - 2) / 2 the fine vertices are, in id order: the n_corner corners; per edge e the vertices s = 1..N-1 counted from lo,
 * at n_corner + e (N - 1) + (s - 1); per triangle t the lattice points (i, j, k), i + j + k = N, all >= 1, numbered by
 * `for j in 1..N-2: for k in 1..N-1-j`, at n_corner + n_edges (N - 1) + t I + index.  n_fine = n_corner + n_edges (N - 1) + n_tri I
 * must be below 2^31.  A lattice point with a zero coordinate lies on an edge and is that edge's vertex: on a -> b (k = 0), j steps
 * from a, s = j if a < b, else N - j; on b -> c (i = 0), k steps from b; on c -> a (j = 0), i steps from c.
 *
 * t4d_tess_faces: out int32 [N^2 n_tri,3].  Triangle t writes rows t N^2 ..: for r = 0..N-1 and s = 0..r, with (i, j, k) =
 * (N - r, r - s, s), the triangle [(i,j,k), (i-1,j+1,k), (i-1,j,k+1)] and, if s < r, [(i,j,k), (i-1,j,k+1), (i,j-1,k+1)] after it.
 * One thread per fine triangle, integer arithmetic only.
 *
 * t4d_tess_points: out float64 [n_fine,dim], dim in {2, 3}, the flat tessellation of values float64 [n_corner,dim]: a corner is
 * copied; an edge vertex is ((N - s) V_lo + s V_hi) / N per component; an interior one ((i A + j B) + k C) / N, (A, B, C) the values
 * at (a, b, c).  The integers are converted to float64 first; the two products are rounded before their sum.
 *
 * t4d_tess_displace: out float64 [n_fine,3] and sampled uint8 [n_fine].  vertices and normals float64 [n_vert,3] (n_vert takes
 * n_corner's place above), uvs float64 [n_uv,2], uv_tri int32 [n_tri,3] the UV corners standing at tri's corners, tri_island int32
 * [n_tri] the label of the triangle's UV island, corner_owner int32 [n_vert] the first corner 3 t + c that names the vertex in
 * row-major order of tri, or -1 for a vertex in no triangle: that vertex is copied through with sampled = 0.  A corner is owned by
 * the triangle of its corner_owner, an edge vertex by the edge's owner, an interior vertex by its own triangle.  Position P and
 * normal n follow t4d_tess_points' rules; so does the UV (u, v), over the owner's UV corners that stand at the same mesh corners (at
 * lo and hi for an edge vertex); L is the owner's tri_island.  len = sqrt(dot3(n, n)); if len is zero or P, n, u, v or len is not
 * finite, out = P and sampled = 0.  Otherwise the code map (code int32 [h,w], low 16 bits; has, labels uint8 [h,w]; 1 <= h, w <=
 * 65536) is sampled at x = u (w - 1), y = (h - v (h - 1)) - 1: x0 = clamp(floor(x), 0, max(w - 2, 0)), x1 = min(x0 + 1, w - 1),
 * fx = clamp(x - x0, 0, 1), and y alike; the taps are (y0,x0), (y0,x1), (y1,x0), (y1,x1) with the weights (1 - fx)(1 - fy),
 * fx (1 - fy), (1 - fx) fy, fx fy; a tap counts where has != 0 and labels == L.  In tap order, S = sum of weight * double(code - 32768)
 * and W = sum of weight, a tap that does not count adding 0.0 to both.  If W > 0, d = (S / W) unit; else if a tap counts, d =
 * (double(sum of code - 32768 over the counting taps) / double(their number)) unit; else d = 0 and sampled = 0.  out_c = P_c +
 * d (n_c / len); sampled = 1 where a tap counted.  unit finite (scan units per code step).  One thread per fine vertex. */
int t4d_tess_faces(const int32_t *tri, const int32_t *tri_edge, int32_t n_tri, int32_t n_corner, int32_t n_edges, int32_t level,
                   int32_t *out, void *hip_stream);
int t4d_tess_points(const double *values, int32_t dim, int32_t n_corner, const int32_t *edges, int32_t n_edges, const int32_t *tri,
                    int32_t n_tri, int32_t level, double *out, void *hip_stream);
int t4d_tess_displace(const double *vertices, const double *normals, const double *uvs, const int32_t *corner_owner,
                      const int32_t *edges, const int32_t *tri, const int32_t *uv_tri, const int32_t *tri_island, int32_t n_vert,
                      int32_t n_uv, int32_t n_edges, int32_t n_tri, int32_t level, const int32_t *code, const uint8_t *has,
                      const uint8_t *labels, int32_t h, int32_t w, double unit, double *out, uint8_t *sampled, void *hip_stream);

/* face.obj of helpers.save_mesh (helpers.py:963-990) on the device (topo4d_amd/objexport.py, csrc/t4d_obj.hip).  Every pointer
 * but `transform` is device memory; none of these synchronises the stream.
 *
 * t4d_obj_vertex_faces: the vertex -> corner CSR of faces [n_faces,3] (once per topology): offsets [n_vert+1], entries [3*n_faces]
 * (corner ids 3*face + k, ascending within a vertex), status [2] = {corners with an index outside [0, n_vert), vertices no face
 * references}.  Scratch: t4d_obj_csr_scratch_bytes.
 * t4d_obj_vertex_normals: trimesh 4.4.1 Trimesh(vertices, faces).vertex_normals in float64 - angle-weighted unit face normals
 * summed in ascending face order, unitised - from vertices [n_vert,3] (float32, or float64 with is_float64 = 1) and the CSR of
 * the same faces.  normals [n_vert,3] float64.  Scratch: t4d_obj_normals_scratch_bytes.
 * t4d_obj_frame_vertices: save_mesh's vertices, out [n_vert,3] float64 = v @ Rg^T + tg, transform (HOST) = Rg row-major then tg
 * (12 doubles); v = float64(means3D) when normals is NULL (frame 1), else means3D pushed along the normal by
 * clamp(sqrt(1 / sum((R^-1 n)^2 / exp(log_scales)^2)), 0, 1e-3) in float32, R = build_rotation(rotations) (external.py:26-43).
 * t4d_obj_format_doubles: repr(float(x)) of values [n] into chars [n, T4D_OBJ_FLOAT_CHARS] (not terminated), lengths [n].
 * t4d_obj_float_lines: "v x y z\n" (kind T4D_OBJ_V, values [rows,3]) or "vt u v\n" (T4D_OBJ_VT, [rows,2]) lines, every value as
 * repr(float) - the f-strings of write_obj_with_uv (helpers.py:258-272) - into out, and the byte count to *out_bytes.
 * t4d_obj_face_lines: "f v+1/uv+1 ...\n" per face; face k's corners are [face_off[k], face_off[k+1]) of v_idx / uv_idx [n_corners]
 * (face_off [n_faces+1] non-decreasing from 0 to n_corners).
 * Output capacity: t4d_obj_text_max_bytes(kind, rows, corners) (rows = lines, corners used by T4D_OBJ_F only); scratch:
 * t4d_obj_text_scratch_bytes with the same arguments. */
#define T4D_OBJ_V 0
#define T4D_OBJ_VT 1
#define T4D_OBJ_F 2
#define T4D_OBJ_FLOAT_CHARS 24
size_t t4d_obj_csr_scratch_bytes(int32_t n_vert);
int t4d_obj_vertex_faces(const int32_t *faces, int64_t n_faces, int32_t n_vert, int32_t *offsets, int32_t *entries, int32_t *status,
                         void *scratch, size_t scratch_bytes, void *hip_stream);
size_t t4d_obj_normals_scratch_bytes(int64_t n_faces);
int t4d_obj_vertex_normals(const void *vertices, int32_t is_float64, int32_t n_vert, const int32_t *faces, int64_t n_faces,
                           const int32_t *offsets, const int32_t *entries, double *normals, void *scratch, size_t scratch_bytes,
                           void *hip_stream);
int t4d_obj_frame_vertices(const float *means3D, const float *log_scales, const float *rotations, const double *normals,
                           int32_t n_vert, const double *transform, double *out, void *hip_stream);
int t4d_obj_format_doubles(const double *values, int64_t n, uint8_t *chars, uint8_t *lengths, void *hip_stream);
size_t t4d_obj_text_max_bytes(int32_t kind, int64_t rows, int64_t corners);
size_t t4d_obj_text_scratch_bytes(int32_t kind, int64_t rows, int64_t corners);
int t4d_obj_float_lines(int32_t kind, const double *values, int64_t rows, uint8_t *out, size_t out_capacity, int64_t *out_bytes,
                        void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_obj_face_lines(const int64_t *face_off, const int64_t *v_idx, const int64_t *uv_idx, int64_t n_faces, int64_t n_corners,
                       uint8_t *out, size_t out_capacity, int64_t *out_bytes, void *scratch, size_t scratch_bytes, void *hip_stream);

/* ---- Ingest: a frame's views from file bytes to float32 targets (csrc/t4d_ingest.hip; topo4d_amd/ingest.py) ----
 * T4DJpegImage: one baseline JPEG (SOF0/SOF1, 8-bit Huffman, 3 components YCbCr, luma sampling 1x1, 2x1 or 2x2 with 1x1 chroma,
 * one interleaved scan) as the host parsed its headers.  Its entropy-coded segment (stuffed, RSTn markers included, up to the
 * marker that ends it) is data[data_offset, data_offset + data_bytes) of the batch's device buffer; the segments of a batch are
 * packed back to back in image order (data_offset = the sum of the previous data_bytes).  quant: the DQT tables in natural
 * order; huff_bits/huff_vals: DHT tables, slots 0-3 DC tables 0-3 and 4-7 AC tables 0-3; comp_*: the table ids of Y, Cb, Cr.
 * The image is written as uint8 [height, width, 3] RGB at out + out_offset, byte-identical to libjpeg-turbo's ISLOW IDCT,
 * fancy upsampling and YCbCr->RGB.  That is libjpeg's C arithmetic, whose 10-bit range table wraps an IDCT output beyond
 * [-512, 511]; libjpeg-turbo's SIMD IDCT (what PIL runs) saturates there.  The two agree, and the output equals PIL's, for
 * blocks whose exact IDCT samples (before the +128 shift) stay within +-500 and whose |coefficient * q| stays below 32768.
 *
 * t4d_jpeg_decode: images (host) and d_images (a device copy of the same array), n of them.  chunk_bits (0: the default 4096,
 * else any value >= 64, byte multiple or not; smaller values are T4D_ERR_ARG) is the length of a lane's chunk in the
 * self-synchronising decode of images without restart intervals.  Every accepted value decodes every valid file: a chunk
 * boundary may fall anywhere, the 1-7 padding bits after the last block included.
 * status[i] (device) receives 0 or an OR of 1 (entropy segment ended early), 2 (more MCUs than the frame holds), 4 (a code no
 * Huffman table holds, or a DHT table that over-fills the code space), 8 (RSTn markers missing, extra or out of sequence).
 * A DHT table that over-fills the code space or lists more than 256 symbols is refused: the image gets bit 4, its table is
 * replaced by one that matches no code, its pixels are unspecified, and the other images of the batch are unaffected.
 * No read outside data[data_offset, data_offset + data_bytes) is made whatever the bytes hold, and scratch may hold anything. */
typedef struct T4DJpegImage {
    int32_t width, height;
    int32_t h_samp, v_samp;
    int32_t restart_interval;               /* MCUs per restart interval, 0: none */
    int32_t reserved0;
    int64_t data_offset, data_bytes;
    int64_t out_offset;
    uint8_t comp_quant[3], comp_dc[3], comp_ac[3];
    uint8_t reserved1[7];
    uint16_t quant[4][64];
    uint8_t huff_bits[8][16];
    uint8_t huff_vals[8][256];
} T4DJpegImage;
size_t t4d_jpeg_scratch_bytes(const T4DJpegImage *images, int32_t n, int32_t chunk_bits);
int t4d_jpeg_decode(const T4DJpegImage *images, const T4DJpegImage *d_images, int32_t n, const uint8_t *data, int32_t chunk_bits,
                    uint8_t *out, size_t out_capacity, int32_t *status, void *scratch, size_t scratch_bytes, void *hip_stream);

/* ---- PNG decode (csrc/t4d_pngdec.hip, csrc/t4d_inflate.h; topo4d_amd/png.py) ----
 * T4DPngImage: one non-interlaced PNG of colour type 0 (grey, 8 or 16 bits), 2 (RGB), 4 (grey + alpha) or 6 (RGBA) at 8 bits, as
 * the host parsed its chunks: channels 1..4, bytes_per_sample 1, or 2 with channels 1.  Its IDAT payloads are the n_chunks rows
 * from first_chunk of the batch's chunk table d_chunks, int64 [n_chunks_total, 2] = (offset into data, bytes), in file order; the
 * images of a batch hold consecutive ranges of the table in image order.  A payload of 0 bytes is legal.  Joined, the payloads are
 * one zlib stream that inflates to height rows of row = 1 + width*channels*bytes_per_sample bytes: a filter byte 0..4, then the
 * filtered row.  The image is written at out + out_offset as uint8 [height, width, channels], or for 16-bit grey as uint16
 * [height, width] in little-endian order (out_offset even), equal to np.array(PIL.Image.open(file)).
 *
 * Two schedules decode a stream.  Chunk-parallel (path 1): one wave per payload decodes it as if it began at a block boundary with
 * no history; the image takes this path when the zlib header and the Adler-32 trailer lie in payloads of their own and every other
 * payload verifies - whole blocks, all bytes consumed, a byte-aligned end after a block end, no distance before its own first byte,
 * at most 65536 bytes made, BFINAL exactly in the last - and the sizes sum to height*row; then the parse is the stream's own.
 * Serial (path 2): any other image, the whole stream by one wave.  path[i] (device) receives 1 or 2.
 * status[i] (device) receives 0 or an OR of the T4D_PNG_ERR_* bits.  No read is made outside the payloads and no write outside
 * the image's height*row bytes of scratch and its bytes of out, whatever the payloads hold; an image with a non-zero status has
 * unspecified pixels.  images is the host copy of d_images; d_chunks, data, out, status, path and scratch are device memory. */
#define T4D_PNG_ERR_END 1      /* the stream ended early, or made more than height*row bytes */
#define T4D_PNG_ERR_BLOCK 2    /* a bad zlib header, block type 3, or a stored block with LEN != ~NLEN */
#define T4D_PNG_ERR_TABLE 4    /* a code table zlib refuses: too many codes, over-subscribed, incomplete, no end-of-block, bad repeat */
#define T4D_PNG_ERR_CODE 8     /* an invalid code, or a distance that reaches before the start of the output */
#define T4D_PNG_ERR_LENGTH 16  /* the stream ended with fewer than height*row bytes */
#define T4D_PNG_ERR_FILTER 32  /* a filter byte above 4 */
#define T4D_PNG_ERR_ADLER 64   /* the Adler-32 of the inflated bytes is not the stream's trailer */
typedef struct T4DPngImage {
    int32_t width, height;
    int32_t channels, bytes_per_sample;
    int32_t first_chunk, n_chunks;
    int64_t out_offset;
} T4DPngImage;
size_t t4d_pngdec_scratch_bytes(const T4DPngImage *images, int32_t n, int32_t n_chunks);
int t4d_png_decode(const T4DPngImage *images, const T4DPngImage *d_images, int32_t n, const int64_t *d_chunks, int32_t n_chunks,
                   const uint8_t *data, uint8_t *out, size_t out_capacity, int32_t *status, int32_t *path, void *scratch,
                   size_t scratch_bytes, void *hip_stream);

/* T4DWarpView: skimage.transform.warp(image, matrix, order=1, mode="constant", cval, clip=True) of one uint8 HWC image read as
 * image / 255.0 in float64, rounded to float32 and written as [channels, out_rows, out_cols] to dst.  src: rows x cols x
 * channels samples, src_pitch bytes per row (a crop of a wider image: src_pitch > cols * channels).  matrix: the first two rows
 * of the inverse map, output (col, row) -> source (col, row).  The output is clipped to the input's [min, max], widened to
 * cval where cval lies outside it and inside the warped values' range (_clip_warp_output).
 * t4d_warp_views: views (host) and d_views (a device copy), one launch set for all of them. */
typedef struct T4DWarpView {
    const uint8_t *src;
    float *dst;
    int32_t rows, cols, channels, src_pitch;
    int32_t out_rows, out_cols;
    double matrix[6];
    double cval;
} T4DWarpView;
size_t t4d_warp_scratch_bytes(int32_t n_views);
int t4d_warp_views(const T4DWarpView *views, const T4DWarpView *d_views, int32_t n_views, void *scratch, size_t scratch_bytes,
                   void *hip_stream);

/* T4DLensView: one capture view undistorted by Metashape's frame-camera model, turned and (optionally) box-filtered down in ONE
 * resampling of a uint8 HWC photograph read as image / 255.0 in float64 (csrc/t4d_lens.h holds the map and the sampling;
 * csrc/t4d_undistort.hip the kernel).  src, rows, cols, channels, src_pitch, dst, out_rows, out_cols as in T4DWarpView.
 * Over a virtual image U of out_rows*supersample x out_cols*supersample:
 *   1. matrix (as in T4DWarpView) takes U's pixel (col, row) to index coordinates (C, R) of the undistorted sensor image;
 *   2. lens = {f, cxa, cya, k1, k2, k3, k4, p1, p2, b1, b2} (pixels of the photograph in src; cxa = width/2 + cx) takes them to
 *      index coordinates (C_src, R_src) of the photograph:  x = ((C + 0.5) - cxa) / f, y likewise, r2 = x*x + y*y,
 *      rad = r2*(k1 + r2*(k2 + r2*(k3 + r2*k4))), dx = x*rad + p1*(r2 + 2*x*x) + 2*p2*x*y, dy = y*rad + p2*(r2 + 2*y*y) + 2*p1*x*y,
 *      C_src = C + f*dx + b1*(x + dx) + b2*(y + dy), R_src = R + f*dy (all coefficients zero: (C, R) exactly);
 *   3. the sample is skimage's order-1 interpolation there (taps outside the photograph are cval), or with nearest != 0 the
 *      single tap at floor(coordinate + 0.5) (label masks); a coordinate more than a sample outside the photograph, or not
 *      finite, gives cval itself;
 *   4. dst[ch, r, c] = float32(sum of U over the supersample x supersample block, row-major, / supersample^2).
 * There is no clip step.  t4d_undistort_views: views (host) and d_views (a device copy), one launch for all of them. */
typedef struct T4DLensView {
    const uint8_t *src;
    float *dst;
    int32_t rows, cols, channels, src_pitch;
    int32_t out_rows, out_cols;
    int32_t supersample;                    /* 1..T4D_LENS_MAX_SUPERSAMPLE */
    int32_t nearest;                        /* 0 or 1 */
    double matrix[6];
    double lens[11];
    double cval;
} T4DLensView;
#define T4D_LENS_MAX_SUPERSAMPLE 64
int t4d_undistort_views(const T4DLensView *views, const T4DLensView *d_views, int32_t n_views, void *hip_stream);

/* ---- JPEG encode (csrc/t4d_jpegenc.hip, csrc/t4d_jpeg_fdct.h; topo4d_amd/jpeg.py, topo4d_amd/prepare.py) ----
 * T4DJpegEncImage: one uint8 [height, width, 3] RGB image on the device, src_pitch bytes per row, 1..65535 pixels a side; its file
 * is written at out + out_offset, and the ranges [out_offset, out_offset + t4d_jpeg_enc_max_bytes) of a batch must not overlap.
 * t4d_jpeg_encode writes n complete baseline JFIF files (SOI, JFIF APP0, two DQT, SOF0, the four Annex K DHT, SOS, one interleaved
 * scan without restart markers, EOI), byte for byte what libjpeg-turbo writes after jpeg_set_quality(quality, TRUE) with
 * luma sampling 1x1 (subsampling 0, 4:4:4), 2x1 (1, 4:2:2) or 2x2 (2, 4:2:0) and JDCT_ISLOW - PIL's
 * save(f, "JPEG", quality=quality, subsampling=subsampling) - and the length of file i to out_bytes[i] (device, int64; -1 if it
 * did not fit, which t4d_jpeg_enc_max_bytes rules out).  The bytes are a pure function of pixels, shape, quality and subsampling;
 * nothing is written beyond a file's length; the stream is not synchronised.  images is the host copy of d_images; scratch may
 * hold anything.  t4d_jpeg_enc_max_bytes / t4d_jpeg_enc_scratch_bytes depend on the shapes alone (0: refused).
 * t4d_views_to_u8: float32 [channels, height, width] -> uint8 [height, width, channels],
 * clip(floor(float64(x) * 255 + 0.5), 0, 255) (NaN: 0): a resampled view as the encoders read it. */
typedef struct T4DJpegEncImage {
    const uint8_t *src;
    int32_t width, height;
    int32_t src_pitch;
    int32_t reserved;
    int64_t out_offset;
} T4DJpegEncImage;
size_t t4d_jpeg_enc_max_bytes(int32_t height, int32_t width, int32_t subsampling);
size_t t4d_jpeg_enc_scratch_bytes(const T4DJpegEncImage *images, int32_t n, int32_t subsampling);
int t4d_jpeg_encode(const T4DJpegEncImage *images, const T4DJpegEncImage *d_images, int32_t n, int32_t quality, int32_t subsampling,
                    uint8_t *out, size_t out_capacity, int64_t *out_bytes, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_views_to_u8(const float *src, int32_t channels, int32_t height, int32_t width, uint8_t *dst, void *hip_stream);

/* ---- Coarse setup: initialize_params' coarse half and initialize_losses' topology (csrc/t4d_setup.hip; topo4d_amd/coarse.py) ----
 * t4d_setup_vertex_colors: compute_vertex_colors (helpers.py:181-209).  image: uint8 [height, width, channels] (3 or 4);
 * corner_uv [n_corners,2] float64: the UV of triangle corner 3*face+k; offsets / entries: t4d_obj_vertex_faces' CSR of the same
 * triangles.  Per corner get_color_from_texture (helpers.py:300-333) in float64; per vertex the integer mean of its corners
 * -> colors [n_vert,3] int32, rgb_colors [n_vert,3] float32 = float32(colors / 255.0).  status [3] (device): corners whose
 * column / row lands outside the image (getpixel would raise; nothing is read), the first such corner (INT32_MAX: none),
 * vertices in no corner.  Scratch: t4d_setup_colors_scratch_bytes.
 * t4d_setup_quaternions: external.build_quaterion (external.py:45-61) in float32 of float32(normals [n,3] float64) -> [n,4].
 * t4d_setup_one_ring: train.py:177-200 for the padded neighbor_indices [n_vert,K] int64 and eye_del [n_vert] (1: in
 * eye_del_masks) -> neighbor_weight, neighbor_dist [n_vert,K] float32; status [1]: indices outside [0, n_vert).
 * t4d_setup_region_weights: out = neighbor_weight with `out[mask_m, :] *= factors[m]` (float32) for m = 0..n_masks-1 in order,
 * each at most once per row; mask m is rows[mask_off[m], mask_off[m+1]) (mask_off on the HOST, d_mask_off its device copy;
 * rows outside [0, n_vert) are ignored).  Scratch: t4d_setup_region_scratch_bytes.
 * t4d_setup_flatten_edges: the FlattenLoss / SoftFlattenLoss constructors (loss_util.py:114-170, 262-318) over faces [F,3] int32
 * and their t4d_obj_vertex_faces CSR, for the candidate edges [n_edges,2] in the host's set order.  out [4, n_edges] int64
 * holds v0s, v1s, v2s, v3s in its first *n_out (device) columns.  status [2] (device): edge ends outside [0, n_vert), faces with
 * no third corner met by an edge of at most two faces (the reference drops an edge of more before it looks at their corners).
 * Scratch: t4d_setup_edges_scratch_bytes.
 * t4d_setup_neighbor_mask: FlattenLoss_v2's mask (loss_util.py:232-241): mask [n_vert,K,3] int64 = (k < neighbor_num[v]). */
#define T4D_SETUP_MAX_MASKS 32
size_t t4d_setup_colors_scratch_bytes(int64_t n_corners);
int t4d_setup_vertex_colors(const uint8_t *image, int32_t width, int32_t height, int32_t channels, const double *corner_uv,
                            int64_t n_corners, const int32_t *offsets, const int32_t *entries, int32_t n_vert, int32_t *colors,
                            float *rgb_colors, int32_t *status, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_setup_quaternions(const double *normals, int32_t n, float *quaternions, void *hip_stream);
int t4d_setup_one_ring(const float *means3D, int32_t n_vert, int32_t K, const int64_t *neighbor_indices, const uint8_t *eye_del,
                       float *neighbor_weight, float *neighbor_dist, int32_t *status, void *hip_stream);
size_t t4d_setup_region_scratch_bytes(int32_t n_vert);
int t4d_setup_region_weights(const float *neighbor_weight, int32_t n_vert, int32_t K, const int32_t *rows, const int32_t *d_mask_off,
                             const int32_t *mask_off, int32_t n_masks, const float *factors, float *out, void *scratch,
                             size_t scratch_bytes, void *hip_stream);
size_t t4d_setup_edges_scratch_bytes(int64_t n_edges);
int t4d_setup_flatten_edges(const int32_t *faces, int32_t n_vert, const int32_t *offsets, const int32_t *entries, const int32_t *edges,
                            int64_t n_edges, int64_t *out, int64_t *n_out, int32_t *status, void *scratch, size_t scratch_bytes,
                            void *hip_stream);
int t4d_setup_neighbor_mask(const int64_t *neighbor_num, int32_t n_vert, int32_t K, int64_t *mask, void *hip_stream);

/* ---- Scoring: a textured mesh rendered into the capture views, and per-view image metrics (csrc/t4d_meshrender.hip;
 * topo4d_amd/meshrender.py) ----
 * t4d_mesh_render: vertices [n_vert,3] float32 in the training world frame, triangles and uv_triangles [n_tri,3] int32 (indices
 * into vertices / uvs [n_uv,2] float32), texture [tex_h,tex_w,3] uint8 (tex_is_float32 = 0, read as x / 255.0) or float32 (1),
 * views [n_views, T4D_VIEW_FLOATS] packed view records of one size h x w, background (HOST) 3 floats.  Outputs: color
 * [n_views,3,h,w] float32, depth [n_views,1,h,w] float32 (0: no triangle), tri_index [n_views,h,w] int32 (-1: no triangle).
 * Rules (reproduced bit for bit by a float64 numpy restatement; everything float64 without FP contraction, outputs rounded once):
 * clip = projmatrix (x,y,z,1), ndc = clip.xyz / clip.w, pixel = ((ndc + 1) S - 1) / 2, view z = (viewmatrix (x,y,z,1)).z; a
 * triangle with a corner at view z <= 0.01 is dropped.  Pixel (x, y) samples the point (x, y); coverage by edge functions of the
 * positively oriented triangle (each evaluated from the lexicographically smaller end of its edge), all >= 0, exact zeros by the
 * top-left rule; zero-area triangles are skipped, none is culled by facing.  depth = 1 / sum(b_i / z_i); a pixel keeps the
 * lexicographic minimum of (float32 bits of the depth, triangle index).  uv = sum beta_i uv_i, beta_i = (b_i / z_i) / sum;
 * texel x = u (tex_w - 1), y = (tex_h - v (tex_h - 1)) - 1, clamped to the texture; bilinear (T4D_MESH_BILINEAR) or nearest
 * with round-half-even (T4D_MESH_NEAREST).  pair_capacity bounds the (triangle, 16x16 tile) pairs over all views; on
 * T4D_ERR_PAIR_OVERFLOW *pairs_needed (host) holds the size to retry with.  Synchronises the stream once.
 * t4d_image_metrics: per view of render / target [n_views,3,h,w] float32, out[v] (device, T4D_METRICS_FIELDS doubles) =
 * { external.calc_psnr(render, target).mean() over the whole image, then over the pixels with coverage >= 0 (coverage
 * [n_views,h,w] int32, e.g. tri_index; NULL: every pixel) and mask > 0.5 (mask [n_views,1,h,w] float32 or NULL): pixel count,
 * mean |d|, mean d^2, PSNR of that mean, mean SSIM (external.calc_ssim's 11x11 window, sigma 1.5, zero padding, map in float32) }.
 * Means run over the three channels; sums are float64 in a fixed order.  Does not synchronise the stream. */
#define T4D_MESH_BILINEAR 0
#define T4D_MESH_NEAREST 1
#define T4D_METRICS_FIELDS 6
size_t t4d_mesh_render_scratch_bytes(int32_t n_views, int32_t n_tri, int32_t h, int32_t w, int64_t pair_capacity);
int t4d_mesh_render(const float *vertices, int32_t n_vert, const int32_t *triangles, const int32_t *uv_triangles, int32_t n_tri,
                    const float *uvs, int32_t n_uv, const void *texture, int32_t tex_is_float32, int32_t tex_h, int32_t tex_w,
                    const float *views, int32_t n_views, int32_t h, int32_t w, const float *background, int32_t mapping,
                    float *color, float *depth, int32_t *tri_index, void *scratch, size_t scratch_bytes, int64_t pair_capacity,
                    int64_t *pairs_needed, void *hip_stream);
size_t t4d_image_metrics_scratch_bytes(int32_t n_views, int32_t h, int32_t w);
int t4d_image_metrics(int32_t n_views, int32_t h, int32_t w, const float *render, const float *target, const float *mask,
                      const int32_t *coverage, double *out, void *scratch, size_t scratch_bytes, void *hip_stream);

/* ---- Projection: the capture photographs gathered into a UV texture (csrc/t4d_projtex.hip; topo4d_amd/projtex.py) ----
 * t4d_project_texture: pos / nrm [tex_h,tex_w,3] float32 (each texel's point in the training world frame and its normal, any
 * length), coverage [tex_h,tex_w] uint8, views [n_views, T4D_VIEW_FLOATS] packed view records of one size h x w (n_views <= 255),
 * photos [n_views,3,h,w] float32, depth [n_views,1,h,w] float32 as t4d_mesh_render writes it (0: no triangle).  Outputs: color
 * [tex_h,tex_w,3] float32, weight [tex_h,tex_w] float32, count [tex_h,tex_w] uint8 (views that contributed).
 * Per covered texel with a non-zero normal, views in ascending order (float64 without FP contraction in the order written down in
 * csrc/t4d_projtex.hip; tests/projtex_ref.py reproduces every output bit): t4d_mesh_render's projection gives the pixel (px, py)
 * and the view depth z; the view is rejected when z <= 0.01, when one of the four bilinear taps at floor(px), floor(py) lies
 * outside the image, when a tap of depth is 0 (background) or z > depth (1 + depth_tol) (a nearer surface), or when cos < cos_min,
 * cos the angle between the unit normal and the unit vector to the camera centre -R^T t of the view matrix (never the record's
 * campos).  Its weight is cos^power (power 0..8, by repeated multiplication) times min(1, m / fade_px), m the distance of (px, py)
 * to the nearest of the lines x = 0, x = w - 1, y = 0, y = h - 1 (fade_px = 0: no fade); a weight that is not > 0 rejects the view
 * too.  Its sample is the bilinear mix of the photograph's taps.  T4D_PROJTEX_WEIGHTED: color = sum(w s) / sum(w), weight =
 * sum(w).  T4D_PROJTEX_BEST: the sample and the weight of the view of largest w, the lowest such view on ties.  Every other texel
 * gets zeros.  Does not synchronise the stream. */
#define T4D_PROJTEX_WEIGHTED 0
#define T4D_PROJTEX_BEST 1
int t4d_project_texture(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w, const float *views,
                        int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth, int32_t power,
                        double cos_min, double fade_px, double depth_tol, int32_t mode, float *color, float *weight, uint8_t *count,
                        void *hip_stream);
/* Equalising the cameras (projtex.pair_stats / solve_gains): exposure and white balance differ from camera to camera, and a blend
 * of unequal cameras shows a step wherever the set of contributing views changes.
 * t4d_project_texture_gains: t4d_project_texture with gains [n_views,3] float64 (device; NULL: none): the sample of view v becomes
 * s[c] = s[c] gains[v][c], one rounded float64 product, before it is blended or kept.  With NULL every output bit is
 * t4d_project_texture's, which forwards here.
 * t4d_projtex_pair_stats: what the gains are solved from.  pos, nrm, coverage, power, cos_min, fade_px, depth_tol as above; views
 * [n_views, T4D_VIEW_FLOATS] with 1 <= n_views <= 32, of any mix of sizes: sizes [n_views,2] int32 (h, w) and the tables photos /
 * depth of n_views device pointers ([3,h_v,w_v] and [h_v,w_v] float32) are device memory.  A view takes part at a covered texel
 * with a non-zero normal when t4d_project_texture would accept it there, cos >= stat_cos_min and every channel of its sample
 * (times gains[v][c] when gains is given) satisfies stat_lo <= s[c] <= stat_hi (a NaN fails; -1024 <= stat_lo <= stat_hi <= 1024):
 * clipped or black samples follow no gain model.  Its integer sample is q[c] = llrint(s[c] 65536), half to even.  For every
 * ordered pair (i, j) of views that both take part at a texel, i == j included: pair_count[i][j] += 1, pair_sum[i][j][c] += q_i[c].
 * pair_count int64 [n_views,n_views] and pair_sum int64 [n_views,n_views,3] (device) are ADDED to: the caller zeroes them, and the
 * statistics of several frames accumulate.  Integer sums: the result does not depend on the order of accumulation
 * (tests/projtex_eq_ref.py reproduces every bit).  Neither call synchronises the stream. */
int t4d_project_texture_gains(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                              const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth,
                              const double *gains, int32_t power, double cos_min, double fade_px, double depth_tol, int32_t mode,
                              float *color, float *weight, uint8_t *count, void *hip_stream);
int t4d_projtex_pair_stats(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                           const float *views, int32_t n_views, const int32_t *sizes, const float *const *photos,
                           const float *const *depth, int32_t power, double cos_min, double fade_px, double depth_tol,
                           double stat_cos_min, double stat_lo, double stat_hi, const double *gains, int64_t *pair_count,
                           int64_t *pair_sum, void *hip_stream);
/* Two bands (projtex.low_band / project_bands; mode "twoband"): the views never register to the pixel, so a blend of all views
 * smears the detail and the single best view shows a step where it changes.  The low frequencies are blended over all views and
 * the detail above them comes from the best view alone (Brown & Lowe's multi-band blending with two bands).  The low-pass runs
 * on the photographs, not in UV space, where it would run across island borders.
 * t4d_projtex_low_band: photos [n_views,3,h,w] float32, depth [n_views,1,h,w] float32 (t4d_mesh_render's; the mask is M = depth
 * > 0), 0 <= radius <= 32 in pixels; low [n_views,3,h,w] float32, not the photographs' own memory.  Per view and channel, in
 * float64 without FP contraction: A[r][c] = the sum over k = -radius .. radius ascending of photos[r][c + k], taken only where
 * 0 <= c + k < w and M[r][c + k] (a tap elsewhere is skipped, so a NaN off the mesh stays out), N1[r][c] the number of these
 * taps; B[r][c] = the sum over k ascending of A[r + k][c] for 0 <= r + k < h, N likewise of N1; low = N > 0 ? float32(B / N) : 0.
 * Only mesh pixels count, so the background never bleeds into the face at its silhouette; across a self-occlusion edge (nose
 * over cheek) the box does mix the two surfaces.  With radius 0, low is photos on M and 0 elsewhere.
 * t4d_project_texture_bands: the inputs of t4d_project_texture_gains and low.  Every view accepted at a texel is sampled as there
 * (s) and, by the same bilinear mix over the same taps of low and the same gain, in its low band (l).  low_color [tex_h,tex_w,3]
 * = sum(w l) / sum(w), weight = sum(w), count as there; high [tex_h,tex_w,3] = s - l (one rounded float64 subtraction) and
 * best_weight [tex_h,tex_w] = w of the view of largest w, the lowest such view on ties.  Every other texel gets zeros.  The
 * texture is low_color + high.  tests/projtex_bands_ref.py reproduces every bit of both.  Neither call synchronises the stream. */
int t4d_projtex_low_band(const float *photos, const float *depth, int32_t n_views, int32_t h, int32_t w, int32_t radius, float *low,
                         void *hip_stream);
int t4d_project_texture_bands(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                              const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *low,
                              const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                              double depth_tol, float *low_color, float *weight, uint8_t *count, float *high, float *best_weight,
                              void *hip_stream);
/* Photo-consistency (projtex.consistency; project / project_bands / project_frame take its mask): a specular highlight, a leak of
 * the occlusion test (hair, lashes, a nose rim the mesh does not model) and transient content in one camera are no gain per
 * camera and no registration error; one view disagrees with a consensus of the others (Waechter et al., "Let There Be Color!").
 * t4d_projtex_consistency: the maps, the views with sizes, the tables photos / depth, the rule's four parameters and gains as
 * t4d_projtex_pair_stats takes them (1 <= n_views <= 32, numbered alike); 0 <= reject_tol <= 4, -1 <= vote_cos_min <= 1,
 * 2 <= min_votes <= 32.  Outputs (device): skip [tex_h,tex_w] uint32, 0 at every texel that is not covered with a non-zero normal,
 * and votes [tex_h,tex_w] uint8.  The rule is in integers, so no order of evaluation changes a bit (tests/projtex_consist_ref.py
 * reproduces both outputs).  Per covered texel with a non-zero normal:
 *   A.1. each view is taken through t4d_project_texture's steps as they stand, the sample times gains[v] when given
 *   A.2. for every accepted view, with s' = s >= 0 ? (s <= 4 ? s : 4) : 0 (a NaN becomes 0): q[c] = llrint(s'[c] 65536)
 *   A.3. a voter is an accepted view with cos >= vote_cos_min; votes = n, their number; if n < min_votes nothing is rejected here
 *   A.4. per channel m[c] = the lower median of the voters' q[c]: the value of the voter of rank (n - 1) / 2 (integer division) in
 *        the order by (q[c], view index) ascending
 *   A.5. an accepted view, voter or not, is an outlier when max_c |q[c] - m[c]| > qt, qt = llrint(reject_tol 65536)
 *   A.6. if every accepted view is an outlier there is no consensus and nothing is rejected; otherwise bit v of skip is set for
 *        every outlier v: at least one accepted view is always kept
 * Known limits: with fewer than min_votes facing views nothing is rejected (the rim of the coverage keeps its highlights); a
 * defect most voters share survives; the threshold is absolute, so it is looser in the shadows than a relative one would be.
 * t4d_project_texture_skip / t4d_project_texture_bands_skip: t4d_project_texture_gains / t4d_project_texture_bands with the mask
 * skip [tex_h,tex_w] uint32 (device; NULL: none, and every output bit is theirs: they forward here): view v of the launch is left
 * out at a texel, exactly as a view that failed the weight test (it adds to no sum, is no candidate for the best view and does
 * not count), when bit skip_base + v of skip[texel] is set; with skip, skip_base >= 0 and skip_base + n_views <= 32.  count is
 * the number of contributing views; under a mask of t4d_projtex_consistency over the same views it never drops to 0 where it was
 * above 0.  No call synchronises the stream. */
int t4d_projtex_consistency(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                            const float *views, int32_t n_views, const int32_t *sizes, const float *const *photos,
                            const float *const *depth, int32_t power, double cos_min, double fade_px, double depth_tol,
                            const double *gains, double reject_tol, double vote_cos_min, int32_t min_votes, uint32_t *skip,
                            uint8_t *votes, void *hip_stream);
int t4d_project_texture_skip(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                             const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth,
                             const double *gains, int32_t power, double cos_min, double fade_px, double depth_tol, int32_t mode,
                             float *color, float *weight, uint8_t *count, const uint32_t *skip, int32_t skip_base, void *hip_stream);
int t4d_project_texture_bands_skip(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                   const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *low,
                                   const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                                   double depth_tol, float *low_color, float *weight, uint8_t *count, float *high,
                                   float *best_weight, const uint32_t *skip, int32_t skip_base, void *hip_stream);
/* Registration (projtex.view_flows; project / project_bands / project_frame take its flows): calibration, the tracked mesh and the
 * lens model are never exact to the pixel, so the views of one frame disagree by a pixel or two.  Each view carries a small 2D
 * flow against the consensus of all views and its photograph is sampled through it (Eisemann et al., "Floating Textures").
 * t4d_project_texture_flow / t4d_project_texture_bands_flow: t4d_project_texture_skip / t4d_project_texture_bands_skip with
 * flows [n_views,h,w,2] int16 (device, aligned to 4 bytes; NULL: none, and every output bit is theirs: they forward here), the
 * pair (f_y, f_x) of a pixel in 1/256 of a photograph pixel, in t4d_drift_dense's component order.  Per covered texel with a
 * non-zero normal and view:
 *   F.1. the view goes through every step of t4d_project_texture at the unshifted pixel (px, py), exactly as it stands: the near
 *        plane, the four taps inside the image, the depth test on the four depth taps, cos >= cos_min, the weight with its edge
 *        fade, and the skip bit.  Geometry decides visibility and weight; the flow only moves the colour sample.
 *   F.2. for an accepted view the flow is read at the nearest pixel iy = (int)floor(py + 0.5), ix = (int)floor(px + 0.5), each
 *        clamped to the image (one 32-bit load)
 *   F.3. px' = px + f_x / 256.0, py' = py + f_y / 256.0, float64 operations
 *   F.4. if one of the four bilinear taps at floor(px'), floor(py') lies outside the image the view is rejected as if F.1 had not
 *        accepted it: it does not count, cannot be the best view and enters no blend
 *   F.5. otherwise its sample is the bilinear mix of the photograph's taps at (px', py'), by the same expression; in the bands
 *        entry the same holds for low.  Gains, blending, the ties of the best view and count are unchanged.
 * tests/projtex_flow_ref.py reproduces every output bit.  Known limits of the flows projtex.view_flows makes: a block straddling a
 * self-occlusion edge matches two surfaces; smooth skin keeps few blocks and falls back to zero flow; a misregistration beyond the
 * search radius is dropped, not corrected.  Neither call synchronises the stream. */
int t4d_project_texture_flow(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                             const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *depth,
                             const double *gains, int32_t power, double cos_min, double fade_px, double depth_tol, int32_t mode,
                             float *color, float *weight, uint8_t *count, const uint32_t *skip, int32_t skip_base, void *hip_stream,
                             const int16_t *flows);
int t4d_project_texture_bands_flow(const float *pos, const float *nrm, const uint8_t *coverage, int32_t tex_h, int32_t tex_w,
                                   const float *views, int32_t n_views, int32_t h, int32_t w, const float *photos, const float *low,
                                   const float *depth, const double *gains, int32_t power, double cos_min, double fade_px,
                                   double depth_tol, float *low_color, float *weight, uint8_t *count, float *high,
                                   float *best_weight, const uint32_t *skip, int32_t skip_base, void *hip_stream,
                                   const int16_t *flows);

/* Exact closest point on a triangle soup, or on a bare point cloud, for many query points (csrc/t4d_closest.hip): what
 * topo4d_amd/scanscore.py scores a frame's face.obj against its multi-view-stereo scan with.  It stands in for
 * trimesh.proximity.closest_point / open3d's RaycastingScene.compute_closest_points on the host; the reference project has no
 * counterpart.  All buffers are device memory unless stated; every call takes the stream last.
 * The primitives are the n_faces triangles `faces` (int32 [n_faces,3], every index in [0, n_vert): the caller checks) of
 * `vertices` (float64 [n_vert,3]), or, with n_faces == 0, the n_vert points themselves.  bbox (host, 6 doubles: min xyz, max xyz
 * of the vertices) and mean_extent (host: the mean over the primitives of the longest side of their axis-aligned box, 0 for
 * points) fix the uniform grid; the same values go to the size query and to the build.
 * t4d_closest_index_bytes: bytes of the index buffer for lists of up to entry_capacity (primitive, cell) entries; 0 on bad
 * arguments.  t4d_closest_build: fills `index`; on T4D_ERR_PAIR_OVERFLOW *entries_needed (host) holds the capacity to retry
 * with.  Synchronises the stream.  The index holds a copy of the primitives: vertices and faces may be freed afterwards.
 * t4d_closest_query: per query point (float64 [n_queries,3]) d2 (float64, squared distance), prim_index (int32) and closest
 * (float64 [n_queries,3]) of the nearest primitive; among primitives of equal d2 the lowest index.  max_dist < 0 or +inf: no
 * limit; otherwise a query is matched iff d2 <= max_dist * max_dist, and an unmatched one gets d2 = +inf, prim_index = -1,
 * closest = 0.  flags: T4D_CLOSEST_INPUT_ORDER walks the queries in input order instead of grouped by grid cell (the same
 * results; kept for measurement).  Uses a work area inside `index`: one query at a time per index.  The result equals a
 * float64 brute force over all primitives with the arithmetic of tests/scanscore_ref.py, bit for bit.
 * t4d_closest_signed: signed_dist[i] = sqrt(d2[i]) with the sign of (p - closest) . ((b - a) x (c - a)) of the chosen
 * triangle; 0 where that is 0, for point primitives and for unmatched queries.
 * t4d_closest_raycast: per ray (origins, dirs: float64 [n_rays,3]) the triangle of a triangle index (a point index is
 * T4D_ERR_ARG) that the line o + t d meets at the smallest |t| within [t_lo, t_hi] (host; finite, with a finite difference):
 * out_t (float64), out_prim (int32) and out_uv (float64 [n_rays,2], the hit is a + u (b - a) + v (c - a)).  scratch as for
 * t4d_closest_query; flags: T4D_CLOSEST_INPUT_ORDER as there, T4D_RAY_SAME_SIDE counts only triangles whose normal
 * (b - a) x (c - a) points along d.  The hit rule, in float64 without contraction and with dot3(u,v) = (u0 v0 + u1 v1) + u2 v2,
 * for ray (o, d) and triangle (a, b, c), in this order:
 *   1. e1 = b - a, e2 = c - a, pv = d x e2, det = dot3(e1, pv); det == 0 is a miss.
 *   2. With T4D_RAY_SAME_SIDE, det >= 0 is a miss.
 *   3. tv = o - a, u = dot3(tv, pv) / det; a miss unless u >= 0 && u <= 1.
 *   4. qv = tv x e1, v = dot3(d, qv) / det; a miss unless v >= 0 && u + v <= 1.
 *   5. t = dot3(e2, qv) / det; a miss unless t >= t_lo && t <= t_hi.
 *   6. Box condition: on every axis k the computed point p_k = o_k + t d_k satisfies p_k >= min(a_k, b_k, c_k) - margin and
 *      p_k <= max(a_k, b_k, c_k) + margin, margin being the grid's (2^-40 of the coordinates' magnitude), else a miss.
 * Quotients, not a reciprocal; a NaN fails every comparison.  Among the hits the smallest |t| wins, then t >= 0 over t < 0,
 * then the lowest triangle index.  A miss writes t = 0, prim = -1, uv = 0; a ray with a non-finite origin or direction, with
 * an all-zero direction, or with t_lo > t_hi misses every triangle.  The box condition is what makes a walk over the grid
 * cells along the ray equal an all-pairs search however ill-conditioned a grazing ray is: a hit's computed point lies in
 * cells that list its triangle.  Equals tests/scanray_ref.py bit for bit.  The interval is cut into at most 1024 pieces of at
 * most a cell each: a reach of more than 1024 cells is walked in pieces that cover many cells at once, correctly but slowly. */
#define T4D_CLOSEST_INPUT_ORDER 1
#define T4D_RAY_SAME_SIDE 2
size_t t4d_closest_index_bytes(int64_t n_vert, int64_t n_faces, const double *bbox, double mean_extent, int64_t entry_capacity);
int t4d_closest_build(const double *vertices, int64_t n_vert, const int32_t *faces, int64_t n_faces, const double *bbox,
                      double mean_extent, void *index, size_t index_bytes, int64_t entry_capacity, int64_t *entries_needed,
                      void *hip_stream);
size_t t4d_closest_query_scratch_bytes(int64_t n_queries);
int t4d_closest_query(void *index, size_t index_bytes, const double *points, int64_t n_queries, double max_dist, int32_t flags,
                      double *d2, int32_t *prim_index, double *closest, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_closest_signed(const void *index, size_t index_bytes, const double *points, int64_t n_queries, const double *d2,
                       const int32_t *prim_index, const double *closest, double *signed_dist, void *hip_stream);
int t4d_closest_raycast(void *index, size_t index_bytes, const double *origins, const double *dirs, int64_t n_rays, double t_lo,
                        double t_hi, int32_t flags, double *out_t, int32_t *out_prim, double *out_uv, void *scratch,
                        size_t scratch_bytes, void *hip_stream);

/* Rigid / similarity alignment of a scan to a mesh by iterated closest points (csrc/t4d_align.hip): the device half of
 * topo4d_amd/scanalign.py.  One iteration moves the scan (t4d_align_transform), asks t4d_closest_query for every moved point's
 * closest point on the mesh, and reduces the pairs into one record of float64 sums (t4d_align_accumulate) that the host solves.
 * Everything is float64 without contraction, dot3(u,v) = (u0 v0 + u1 v1) + u2 v2, and every output is a function of the inputs
 * alone; tests/scanalign_ref.py states both in numpy, bit for bit.  Device buffers unless stated; the stream comes last.
 * t4d_align_transform: out[i] = M p[i] + t for n_points float64 [n,3] points; matrix (host, 12 doubles) holds the rows
 * (m0 m1 m2 t) of [M | t], finite, M any 3x3 (a scale included).  Each component is ((m0 x + m1 y) + m2 z) + t.  out may be
 * points.  n_points == 0 is T4D_OK.
 * t4d_align_accumulate: points are the moved points and d2, prim_index, closest what t4d_closest_query gave for them on the
 * triangle index `index` (an index of bare points is T4D_ERR_ARG).  Per pair, with (a, b, c) the corners of triangle prim_index
 * as the index holds them: e = p - closest, n = (b - a) x (c - a) (the products of t4d_closest_signed), nn = dot3(n, n).  The
 * pair's class is the first that applies:
 *   unmatched   prim_index < 0 (or beyond the index's triangles)
 *   gated       gate2 >= 0 and d2 > gate2 (gate2 < 0: no gate; d2 == gate2 is kept)
 *   degenerate  nn == 0
 *   off-normal  d2 > 0 and en * en < (cos2 * d2) * nn, en = dot3(e, n): the residual lies across the surface, as it does for a
 *               point whose closest point sits on an open rim of the mesh
 *   kept        every other pair
 * A kept pair adds, with s = sqrt(nn), nh = n / s (three quotients), r = dot3(e, nh), q = p - origin, g = closest - origin
 * (origin: host, 3 finite doubles), x = q x nh = (q1 nh2 - q2 nh1, q2 nh0 - q0 nh2, q0 nh1 - q1 nh0) and J = (x, nh):
 *   record[T4D_ALIGN_SUM_D2] += d2                       record[T4D_ALIGN_SUM_R2] += r r
 *   record[T4D_ALIGN_JTR + i] += r J[i]                  record[T4D_ALIGN_JTJ + k] += J[i] J[j], k counting i <= j row by row
 *   record[T4D_ALIGN_SUM_Q + i] += q[i]                  record[T4D_ALIGN_SUM_G + i] += g[i]
 *   record[T4D_ALIGN_SUM_QG + 3 i + j] += q[i] g[j]      record[T4D_ALIGN_SUM_QQ] += dot3(q, q), [T4D_ALIGN_SUM_GG] += dot3(g, g)
 * and every pair adds 1 to record[T4D_ALIGN_COUNT + class] (float64 as the sums: exact below 2^53).  That is the point-to-plane
 * Gauss-Newton system (JTJ, JTR) and the Kabsch / Umeyama system of one pass.  record: T4D_ALIGN_RECORD_DOUBLES doubles.
 * Reduction order, fixed: G = min(ceil(n / 256), T4D_ALIGN_MAX_GROUPS) workgroups of 256 lanes; lane l of all L = 256 G adds
 * the pairs l, l + L, l + 2 L, ... to zeros, in that order; within each wave of 64 lanes v[t] = v[t] + v[t + w] for
 * w = 32, 16, 8, 4, 2, 1; a workgroup's four waves give (w0 + w1) + (w2 + w3); a second launch adds the G workgroup sums to
 * zeros in index order.  No atomics.  n_points == 0 writes a record of zeros.  scratch: t4d_align_scratch_bytes(n_points)
 * bytes (0 and a message for n_points < 0 or >= 2^30).
 * Refused before anything touches a device: NULL buffers, a negative count, scratch too small (T4D_ERR_STATE_SIZE), a gate2 or
 * cos2 that is not finite, cos2 outside [0, 1], a matrix or origin that is not finite. */
#define T4D_ALIGN_RECORD_DOUBLES 51
#define T4D_ALIGN_MAX_GROUPS 1024
#define T4D_ALIGN_COUNT 0       /* unmatched, gated, degenerate, off-normal, kept */
#define T4D_ALIGN_SUM_D2 5
#define T4D_ALIGN_SUM_R2 6
#define T4D_ALIGN_JTR 7
#define T4D_ALIGN_JTJ 13
#define T4D_ALIGN_SUM_Q 34
#define T4D_ALIGN_SUM_G 37
#define T4D_ALIGN_SUM_QG 40
#define T4D_ALIGN_SUM_QQ 49
#define T4D_ALIGN_SUM_GG 50
int t4d_align_transform(const double *points, int64_t n_points, const double *matrix, double *out, void *hip_stream);
size_t t4d_align_scratch_bytes(int64_t n_points);
int t4d_align_accumulate(const void *index, size_t index_bytes, const double *points, int64_t n_points, const double *d2,
                         const int32_t *prim_index, const double *closest, const double *origin, double gate2, double cos2,
                         double *record, void *scratch, size_t scratch_bytes, void *hip_stream);

/* Optional per-kernel timing with HIP events recorded on the stream the kernels are launched on.  Between
 * t4d_profile_begin() and t4d_profile_end() every kernel launch of this library is bracketed by two events;
 * t4d_profile_end() synchronises them and returns, per kernel, the summed elapsed time and the launch count.
 * bench.py uses this for the `roofline` object (duration of the dominant kernel).  Not thread-safe. */
typedef struct T4DKernelTime {
    const char *name;
    double total_ms;
    int64_t launches;
} T4DKernelTime;
int t4d_profile_begin(void);
int t4d_profile_end(T4DKernelTime *out, int max_entries, int *n_entries);

/* Test/debug only: byte offsets of the arrays inside a state buffer, in this order:
 *   status, view_total, view_cursor, tile_count, bucket_fill, tile_off, xy, depth, conic_opacity, rgb, clamped,
 *   pair_off, keys, final_T, n_contrib, total_bytes.
 * The layout is NOT part of the stable ABI; tests use it to check the integer state (tile bins, sort order,
 * n_contrib) bit-for-bit against the oracle. */
#define T4D_DEBUG_LAYOUT_FIELDS 16
int t4d_debug_state_layout(const T4DProblem *prob, int has_sh, uint64_t *offsets, int n);

/* Non-rigid fit of a template mesh to a scan (csrc/t4d_nricp.hip): the device half of topo4d_amd/startup.py, after Amberg,
 * Romdhani and Vetter, "Optimal Step Nonrigid ICP" (CVPR 2007).  The host route this stands in for is
 * trimesh.registration.nricp_amberg; the reference project has no counterpart (its README asks for a fitted face_v5.obj).
 * Everything is float64 without contraction, dot3(u,v) = (u0 v0 + u1 v1) + u2 v2, no atomics, and every output is a function of
 * the inputs alone; tests/startup_ref.py states every rule in numpy, bit for bit.  Device buffers unless stated; the stream
 * comes last.  n is the number of template vertices, 1 <= n < 2^30 (n == 0 is T4D_OK and touches nothing).
 *
 * Unknowns.  One 4x3 matrix X_i per vertex; the moved vertex is p_i = X_i^T vt_i with vt_i = (v_i, 1) and v_i the pre-aligned
 * template vertex in the normalised frame (the host's business).  A "field" holds one double per entry of every X_i as
 * [3][4][n]: field[(4 c + r) n + i] is row r of coordinate column c of vertex i.  X, the right-hand side B, the residual R,
 * the preconditioned residual Z, the direction P and K P are fields.  v is float64 [n,3].  The mesh's edges come as the CSR of
 * every vertex's neighbours in ascending index: nbr_off int32 [n + 1], nbr int32 [nbr_off[n]], every entry in [0, n) (the
 * caller checks); deg_i = nbr_off[i + 1] - nbr_off[i].
 *
 * The system of one outer step, per coordinate column c, with a2 = alpha^2, a2g = a2 gamma^2 (host doubles, finite, > 0),
 * g_r = a2 for the rows r = 0, 1, 2 and a2g for r = 3, and s_i the vertex's data weight (float64 [n], >= 0):
 *   (K P)_i[c][r] = g_r * L + d_r,   L = the sum over j in N(i), ascending, added to 0 in that order, of (P_i[c][r] - P_j[c][r]),
 *                   t = ((v0 P_i[c][0] + v1 P_i[c][1]) + v2 P_i[c][2]) + P_i[c][3],  d = s_i * t,  d_r = v_r * d (r < 3), d_3 = d.
 * t4d_nricp_assemble: s_i = w_i + bl_i with bl_i = beta2 * lw_i (lw NULL: bl_i = 0; beta2 host, finite, >= 0; w the data
 * weights t4d_nricp_classify wrote, lw float64 [n] the landmark indicator or weight), the right-hand side
 *   B_i[c][r] = vt_r * (w_i * c_i[c] + bl_i * lt_i[c])   (c: float64 [n,3] targets, lt: float64 [n,3] landmark targets; vt_3 = 1)
 * and the Cholesky factor of the preconditioner's block M_i = diag(deg_i g_r) + s_i vt_i vt_i^T: A[r][q] = (s_i * vt_r) * vt_q
 * for q <= r, A[r][r] = A[r][r] + deg_i * g_r, then for j = 0..3: L[j][j] = sqrt(A[j][j] - sum_{k<j} L[j][k] L[j][k]) and for
 * i > j: L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j], every sum taken by subtracting the products from the first
 * term in ascending k.  A vertex without an edge (deg_i == 0) takes the identity: without data its block is zero, and with data
 * it has rank one.  chol: float64 [10][n], entry r (r + 1) / 2 + q of L[r][q].  Outputs s, B, chol.
 * t4d_nricp_precond: Z = M^-1 R per vertex and column: y_r = (R_r - sum_{k<r} L[r][k] y_k) / L[r][r] for r = 0..3, then
 * z_r = (y_r - sum_{k>r} L[k][r] z_k) / L[r][r] for r = 3..0, sums as above in ascending k.  Quotients, no reciprocal.
 * t4d_nricp_apply: Q = K P and dots[c] = P[c] . Q[c] (device, 3 doubles) by the reduction below over the per-vertex terms
 * ((P0 Q0 + P1 Q1) + P2 Q2) + P3 Q3 of column c.
 *
 * Reduction order, fixed, for every sum over the vertices (the scheme of t4d_align_accumulate): G = min(ceil(n / 256),
 * T4D_NRICP_MAX_GROUPS) workgroups of 256 lanes; lane l of all 256 G adds the vertices l, l + 256 G, ... to zeros in that order;
 * a wave of 64 folds v[t] = v[t] + v[t + w] for w = 32 .. 1; a workgroup's four waves give (w0 + w1) + (w2 + w3); the G
 * workgroup sums are added to zeros in index order.  The largest move is a maximum, exact in any order.
 *
 * Conjugate gradients, the three columns in lock-step, each with its own scalars.  state: T4D_NRICP_STATE_DOUBLES doubles, two
 * records of 16 (record k & 1 is current after k iterations) and ||B[c]||^2 at T4D_NRICP_STATE_BB.  A record holds, per column,
 * rz = R . Z at T4D_NRICP_RZ, rr = R . R at T4D_NRICP_RR, the last pq = P . K P at T4D_NRICP_PQ, the last step alpha at
 * T4D_NRICP_ALPHA and beta at T4D_NRICP_BETA, and the iteration count at T4D_NRICP_ITER.
 * t4d_nricp_cg_start: R = B - K X, Z = M^-1 R, P = Z, and record 0 with rz, rr (pq, alpha, beta, count 0) and bb.
 * t4d_nricp_cg_run: `iters` iterations (0..T4D_NRICP_MAX_RUN) after the `done` (>= 0) already made, three launches each:
 *   1. Q = K P with the workgroup sums of P . Q.
 *   2. pq = those sums in index order; alpha_c = 0 if bit c of stop_mask is set or pq_c == 0, else rz_c / pq_c;
 *      X = X + alpha P, R = R - alpha Q, Z = M^-1 R, with the workgroup sums of R . Z and R . R.
 *   3. rz', rr' = those sums in index order; beta_c = 0 if alpha_c == 0, else rz'_c / rz_c; P = Z + beta P; the next record.
 * A column with alpha = 0 is frozen: X and R keep their bits, no quotient with a zero denominator is taken, nothing is NaN.  A
 * zero right-hand side from X = 0 is such a column (rz == 0 gives alpha == 0).  The host reads `state` when it wants to and
 * sets stop_mask; plain launches only.
 * t4d_nricp_positions: pos_i[c] = ((v0 X_i[c][0] + v1 X_i[c][1]) + v2 X_i[c][2]) + X_i[c][3] (float64 [n,3]) and
 * *move2 (device) = the largest dot3(e, e), e = pos_i - prev_i, over the vertices (prev: float64 [n,3]; NULL: move2 = 0; prev
 * may be pos).
 *
 * t4d_nricp_classify: points are the current p_i and d2, prim_index, closest what t4d_closest_query gave for them on `index`
 * (of the scan, triangles or bare points).  With (a, b, c) the chosen triangle, nv = (b - a) x (c - a), nn = dot3(nv, nv),
 * e = p - closest, en = dot3(e, nv), the class is the first that applies:
 *   0 unmatched    prim_index < 0 (or beyond the index's primitives)
 *   1 gated        gate2 >= 0 and d2 > gate2 (d2 == gate2 is kept)
 *   2 degenerate   triangles only: nn == 0
 *   3 off_normal   triangles only: d2 > 0 and en * en < (cos2 * d2) * nn (a closest point on the scan's open rim)
 *   4 flipped      triangles only, normals not NULL: dot3(m, nh) < normal_cos with m the vertex normal (float64 [n,3]) and
 *                  nh = nv / sqrt(nn) (three quotients); equality is kept
 *   5 weightless   weights not NULL and weights[i] == 0
 *   6 kept
 * Outputs: cls int32 [n]; w float64 [n] = weights[i] (1 without weights) if kept, else 0; target float64 [n,3] = closest if
 * kept, else 0; record (T4D_NRICP_RECORD_DOUBLES doubles): the class counts at 0..6 and the sum of d2 over the kept at
 * T4D_NRICP_SUM_D2, by the reduction above.
 *
 * scratch: t4d_nricp_scratch_bytes(n) bytes for every call that takes one (0 and a message for n < 0 or >= 2^30).
 * Refused before anything touches a device: NULL buffers, a count out of range, scratch too small (T4D_ERR_STATE_SIZE), a
 * scalar that is not finite, a2 or a2g <= 0, beta2 < 0, cos2 or normal_cos outside [0, 1] / [-1, 1], iters or done out of range,
 * stop_mask outside 0..7. */
#define T4D_NRICP_MAX_GROUPS 1024
#define T4D_NRICP_RECORD_DOUBLES 8
#define T4D_NRICP_SUM_D2 7
#define T4D_NRICP_STATE_DOUBLES 40
#define T4D_NRICP_RZ 0
#define T4D_NRICP_RR 3
#define T4D_NRICP_PQ 6
#define T4D_NRICP_ALPHA 9
#define T4D_NRICP_BETA 12
#define T4D_NRICP_ITER 15
#define T4D_NRICP_STATE_BB 32
#define T4D_NRICP_MAX_RUN 4096
size_t t4d_nricp_scratch_bytes(int64_t n);
int t4d_nricp_classify(const void *index, size_t index_bytes, const double *points, int64_t n, const double *d2,
                       const int32_t *prim_index, const double *closest, const double *normals, const double *weights,
                       double gate2, double cos2, double normal_cos, int32_t *cls, double *w, double *target, double *record,
                       void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_nricp_assemble(const double *v, int64_t n, const int32_t *nbr_off, const double *w, const double *c, const double *lw,
                       const double *lt, double a2, double a2g, double beta2, double *s, double *b, double *chol,
                       void *hip_stream);
int t4d_nricp_precond(const double *chol, int64_t n, const double *r, double *z, void *hip_stream);
int t4d_nricp_apply(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2, double a2g,
                    const double *p, double *q, double *dots, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_nricp_cg_start(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2,
                       double a2g, const double *chol, const double *b, const double *x, double *r, double *z, double *p,
                       double *q, double *state, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_nricp_cg_run(const double *v, int64_t n, const int32_t *nbr_off, const int32_t *nbr, const double *s, double a2,
                     double a2g, const double *chol, double *x, double *r, double *z, double *p, double *q, double *state,
                     int32_t done, int32_t iters, int32_t stop_mask, void *scratch, size_t scratch_bytes, void *hip_stream);
int t4d_nricp_positions(const double *v, int64_t n, const double *x, const double *prev, double *pos, double *move2,
                        void *scratch, size_t scratch_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TOPO4D_RASTER_H */
