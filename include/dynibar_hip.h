/* dynibar_hip.h -- C ABI of libdynibar_hip.so: the MI355X (gfx950) per-ray renderer kernels.
 *
 * The reference (google/dynibar) has no FFI layer: its hot path is Python calling PyTorch eager ops.  Each entry
 * point below replaces one group of those op sites; the citation gives the reference lines (paths under
 * /root/reference/ibrnet/).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions: every pointer is a DEVICE pointer to contiguous fp32 (or int32 where noted) unless marked HOST;
 * `stream` is a hipStream_t passed as void*; calls are stream-ordered, allocate nothing and keep no global state;
 * return 0 on success or a negative DYN_E_* code, with a message available from dyn_last_error().
 * All tensors are row-major with the shapes written next to each field.
 */
#ifndef DYNIBAR_HIP_H_
#define DYNIBAR_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYN_ABI_VERSION 1
#define DYN_E_INVALID (-1)  /* bad argument (NULL pointer, unsupported shape) */
#define DYN_E_LAUNCH (-2)   /* HIP launch error */

int dyn_abi_version(void);
const char* dyn_last_error(void);

/* ---- a8 (projection.py:42-47) camera preparation ----------------------------------------------------------
 * cams [V,34] = [h, w, K(4x4), c2w(4x4)] -> proj [V,16]: rows 0..2 of K.inv(c2w) (12 floats), then the source camera
 * centre c2w[:3,3] (3 floats), then 0.  query_cam [34] -> query_center[4] (c2w[:3,3], 0).  Replaces torch.inverse+bmm. */
int dyn_prepare_cameras(const float* cams, int V, const float* query_cam, float* proj, float* query_center, void* stream);

/* ---- featmaps [V,F,Hf,Wf] (NCHW, feature_network.py:302-311) -> channels-last [V,Hf,Wf,F] for 128-byte taps --- */
int dyn_nchw_to_nhwc(const float* src, float* dst, int V, int F, int Hf, int Wf, void* stream);

/* ---- a5 sample_along_camera_ray (render_ray.py:67-131) -------------------------------------------------------
 * depth_range: DEVICE [2] = (near, far).  t_rand: [R,S] uniform draws for det=False, NULL for det=True (the host owns the
 * RNG so tests can inject the reference's draws).  Outputs z_vals [R,S], s_vals [R,S] (may be NULL), pts [R,S,3] (may be NULL). */
typedef struct {
  int R, S;
  int inv_uniform;
  const float* ray_o;       /* [R,3] */
  const float* ray_d;       /* [R,3] */
  const float* depth_range; /* [2] */
  const float* t_rand;      /* [R,S] or NULL */
  float* z_vals;            /* [R,S] */
  float* s_vals;            /* [R,S] or NULL */
  float* pts;               /* [R,S,3] or NULL */
} DynSampleParams;
int dyn_sample_along_ray(const DynSampleParams* p, void* stream);

/* ---- z_vals -> pts, s_vals for the fine pass (render_ray.py:822-831, z_to_s :399-404) ---------------------- */
int dyn_points_from_z(const float* ray_o, const float* ray_d, const float* z_vals, const float* depth_range, int R, int S,
                      float* pts, float* s_vals, void* stream);

/* ---- a8-a11 Projector.compute_with_motions (projection.py:103-176), fused ----------------------------------
 * One kernel: K.inv(c2w) projection, clamp, in-front/in-bounds mask, bilinear zero-padded align_corners taps of the
 * RGB images and of the feature maps at the same normalised location, ray-direction difference.
 * Sample points come either from (ray_o, ray_d, z_vals) [pts_st = o + z d] or from an explicit pts_st array; the
 * per-view points xyz are pts_st itself (static branch, xyz = NULL), an explicit [V,R,S,3] array (scene motion) or -- traj_coeff != NULL, the fused form of
 * compute_traj_pts (render_ray.py:361-369, :691-725) -- formed in the kernel from the motion coefficients: view v sees pts_st + (traj(traj_rows[v]) - traj(traj_ref)),
 * traj(row)[a] = sum_b coeff[.., a B + b] basis[row, b], a negative row = no displacement (virtual views); the same arithmetic, bit for bit, as dyn_trajectory_points,
 * whose [V,R,S,3] output then never exists.  traj_rows is a DEVICE array of V ints. */
typedef struct {
  int R, S, V;
  int H, W;                 /* source image size (tensor dims) */
  int Hf, Wf, F;            /* feature map size / channels (F % 4 == 0) */
  float img_h, img_w;       /* train_cameras[0][:2], used by normalize()/inbound() (projection.py:136) */
  const float* ray_o;       /* [R,3]   (used when pts_st == NULL) */
  const float* ray_d;       /* [R,3] */
  const float* z_vals;      /* [R,S] */
  const float* pts_st;      /* [R,S,3] or NULL */
  const float* xyz;         /* [V,R,S,3] or NULL */
  const float* proj;        /* [V,16] from dyn_prepare_cameras */
  const float* query_center;/* [4] */
  const float* src_rgb;     /* [V,H,W,3] */
  const float* feat_cl;     /* [V,Hf,Wf,F] channels-last */
  float* rgb_feat;          /* [R,S,V,3+F] */
  float* ray_diff;          /* [R,S,V,4], or NULL when the caller has no use for it (the dynamic branch: DynibarDynamic takes none) */
  float* mask;              /* [R,S,V] (the reference's trailing singleton dim is a view) */
  float* pix_mask;          /* [R,S] or NULL: 1 where more than pix_mask_thresh views see the sample (render_ray.py:736-741), else 0 */
  float pix_mask_thresh;
  const float* traj_coeff;  /* [R,S,3 B] or NULL (then the fields below are ignored); needs pts_st, excludes xyz */
  const float* traj_basis;  /* [frames, B] */
  const int* traj_rows;     /* DEVICE [V]: basis row of each view, negative = the undisplaced point */
  int traj_B, traj_ref;     /* basis functions per axis; basis row of the reference time */
} DynProjectGatherParams;
int dyn_project_gather(const DynProjectGatherParams* p, void* stream);

/* ---- a20/a21 raw2outputs_vanilla / raw2outputs (render_ray.py:134-330): one wavefront per ray ------------------
 * raw_static == NULL selects the vanilla (single-branch) form.  pix_mask_*: [R,S] 0/1 floats (the "at least 2 observations"
 * sample masks).  Per-sample outputs may be NULL when the caller does not need them. */
typedef struct {
  int R, S;
  const float* raw_dy;      /* [R,S,4]  (vanilla: the single raw input) */
  const float* raw_static;  /* [R,S,4] or NULL */
  const float* z_vals;      /* [R,S] */
  const float* pix_mask_dy; /* [R,S] */
  const float* pix_mask_st; /* [R,S] or NULL */
  float* rgb;               /* [R,3] */
  float* rgb_static;        /* [R,3] or NULL */
  float* rgb_dy;            /* [R,3] or NULL */
  float* depth;             /* [R] */
  float* ray_mask;          /* [R] 0/1 */
  float* weights;           /* [R,S] */
  float* alpha;             /* [R,S] or NULL */
  float* alpha_dy;          /* [R,S] or NULL */
  float* weights_dy;        /* [R,S] or NULL */
  float* weights_st;        /* [R,S] or NULL */
} DynCompositeParams;
int dyn_composite(const DynCompositeParams* p, void* stream);

/* ---- sample masks: pixel_mask[r,s] = (sum_v mask[r,s,v]) > thresh (render_ray.py:736-741) -------------------- */
int dyn_sample_mask(const float* mask, int RS, int V, float thresh, float* pix_mask, void* stream);

/* ---- a6/a7 fine-sample assembly (render_ray.py:19-64, :790-821): pdf -> cdf -> inverse-CDF -> merge + sort ----
 * weights: coarse weights [R,S]; the kernel drops the two end samples, adds 1e-5, builds the cdf with a sequential
 * per-ray prefix sum accumulated in double and rounded to fp32 per element (what torch.cumsum does on the CPU), inverts it at u (NULL = linspace(0,1,N) i.e. det=True) with the
 * reference's count-of-(u >= cdf_i) rule, and writes the sorted union of coarse and new depths.  inds (optional) returns
 * the reference's `above_inds` for the bit-exact index check. */
typedef struct {
  int R, S, N;              /* S coarse samples, N = N_importance */
  int inv_uniform;
  const float* z_vals;      /* [R,S] */
  const float* weights;     /* [R,S] */
  const float* u;           /* [R,N] or NULL */
  float* z_out;             /* [R,S+N] sorted ascending */
  float* z_samples;         /* [R,N] or NULL: the new depths before the sort */
  int32_t* inds;            /* [R,N] or NULL */
} DynFineSampleParams;
int dyn_fine_samples(const DynFineSampleParams* p, void* stream);

/* ---- a17 DynibarStatic.forward (mlp_network.py:423-527) incl. a12 Pluecker coordinates (render_ray.py:372-396), a13 Fourier
 * features (:530-555), a18 ray attention (:13-31,:56-104), a19 weighted mean/variance over views (:115-119) ----------------
 * Weights: dyn_static_net_pack re-lays the module's state dict out as MFMA operand tiles.  `tensors` are HOST pointers to the
 * row-major fp32 tensors in this order (state-dict names):
 *   ray_dir_fc.0.weight .0.bias ray_dir_fc.2.weight .2.bias ref_feature_fc.0.weight .0.bias base_fc.0.weight .0.bias base_fc.2.weight
 *   .2.bias vis_fc.0.weight .0.bias vis_fc.2.weight .2.bias vis_fc2.0.weight .0.bias vis_fc2.2.weight .2.bias geometry_fc.0.weight
 *   .0.bias geometry_fc.2.weight .2.bias ray_attention.w_qs.weight ray_attention.w_ks.weight ray_attention.w_vs.weight
 *   ray_attention.fc.weight ray_attention.layer_norm.weight ray_attention.layer_norm.bias out_geometry_fc.0.weight .0.bias
 *   out_geometry_fc.2.weight .2.bias rgb_fc.0.weight .0.bias rgb_fc.2.weight .2.bias rgb_fc.4.weight .4.bias s
 * (39 tensors).  F = feature channels of the maps (must be 32).  blob: HOST buffer of dyn_static_net_blob_floats() floats; the
 * caller copies it to the device once per model. */
#define DYN_STATIC_NUM_TENSORS 39
size_t dyn_static_net_blob_floats(void);
int dyn_static_net_pack(const float* const* tensors, int F, float* blob, size_t blob_floats);
size_t dyn_static_net_workspace_bytes(int R, int S, int V);
typedef struct {
  int R, S, V;               /* rays, samples per ray (<= 256), source views (<= 32) */
  int anti_alias_pooling;    /* args.anti_alias_pooling (mlp_network.py:462) */
  int mask_rgb;              /* args.mask_rgb (:457) */
  const float* blob;         /* DEVICE copy of the packed weights */
  const float* ray_o;        /* [R,3] */
  const float* ray_d;        /* [R,3] */
  const float* pts;          /* [R,S,3] */
  const float* rgb_feat;     /* [R,S,V,35] from dyn_project_gather */
  const float* ray_diff;     /* [R,S,V,4] */
  const float* mask;         /* [R,S,V] */
  const float* centers;      /* [V,16]: the proj array of dyn_prepare_cameras (source camera centres at [12..14]) */
  float* raw;                /* [R,S,4] = (r, g, b, sigma) */
  void* workspace;           /* DEVICE scratch of dyn_static_net_workspace_bytes(R,S,V) bytes */
  size_t workspace_bytes;
} DynStaticNetParams;
int dyn_static_net(const DynStaticNetParams* p, void* stream);

/* ---- a16 DynibarDynamic.forward (mlp_network.py:236-316) ---------------------------------------------------------------
 * tensors for dyn_dynamic_net_pack (HOST pointers, state-dict names, 40 tensors):
 *   ray_dir_fc.0.weight .0.bias ray_dir_fc.2.weight .2.bias base_fc.0.weight .0.bias base_fc.2.weight .2.bias vis_fc.0.weight .0.bias
 *   vis_fc.2.weight .2.bias vis_fc2.0.weight .0.bias vis_fc2.2.weight .2.bias geometry_fc.0.weight .0.bias geometry_fc.2.weight .2.bias
 *   ray_attention.w_qs.weight ray_attention.w_ks.weight ray_attention.w_vs.weight ray_attention.fc.weight
 *   ray_attention.layer_norm.weight ray_attention.layer_norm.bias ref_pts_fc.0.weight .0.bias ref_pts_fc.2.weight .2.bias
 *   out_geometry_fc.0.weight .0.bias out_geometry_fc.2.weight .2.bias rgb_fc.0.weight .0.bias rgb_fc.2.weight .2.bias rgb_fc.4.weight .4.bias
 * The net ignores ray_diff and time_diff (anti_alias_pooling is hard-wired off, mlp_network.py:135), so they are not inputs. */
#define DYN_DYNAMIC_NUM_TENSORS 40
size_t dyn_dynamic_net_blob_floats(void);
int dyn_dynamic_net_pack(const float* const* tensors, int F, float* blob, size_t blob_floats);
size_t dyn_dynamic_net_workspace_bytes(int R, int S, int V);
typedef struct {
  int R, S, V;               /* rays, samples per ray (<= 256; must equal the module's n_samples), source views (<= 32) */
  float shift;               /* subtracted from sigma (DynibarMono builds its dynamic net with shift = 5, model.py:307) */
  const float* blob;         /* DEVICE copy of the packed weights */
  const float* ray_d;        /* [R,3] (normalised in the kernel, render_ray.py:655) */
  const float* pts;          /* [R,S,3] reference-time sample points */
  const float* rgb_feat;     /* [R,S,V,35] */
  const float* mask;         /* [R,S,V] */
  const float* time;         /* DEVICE [1]: reference time embedding */
  float* raw;                /* [R,S,4] */
  void* workspace;           /* DEVICE scratch of dyn_dynamic_net_workspace_bytes(R,S,V) bytes */
  size_t workspace_bytes;
} DynDynamicNetParams;
int dyn_dynamic_net(const DynDynamicNetParams* p, void* stream);

/* ---- a14 MotionMLP.forward (mlp_network.py:605-618) + the zeroing of the last samples' coefficients (render_ray.py:684) -------
 * tensors for dyn_motion_mlp_pack (HOST, 18 tensors): pts_linears.0.weight .0.bias ... pts_linears.7.weight .7.bias
 * coeff_linear.weight coeff_linear.bias.   coeff: [R,S,3*num_basis].  n_zero_last = int(round(S * 0.1)). */
#define DYN_MOTION_NUM_TENSORS 18
size_t dyn_motion_mlp_blob_floats(void);
int dyn_motion_mlp_pack(const float* const* tensors, int num_basis, float* blob, size_t blob_floats);
int dyn_motion_mlp(const float* blob, const float* pts, const float* time, int R, int S, int num_basis, int n_zero_last, float sf_mag_div,
                   float* coeff, void* stream);

/* ---- a15 compute_traj_pts + the per-view displaced points (render_ray.py:361-369, :686-709) -------------------------------
 * pts_seq[v] = pts + (traj(row_v) - traj(row_ref)), traj(row) = (sum_b cx_b basis[row,b], sum_b cy_b .., sum_b cz_b ..);
 * rows: HOST array of n_rows basis-row indices (frame + offset); a row index < 0 means "no motion" (virtual views, :988-989).
 * basis: DEVICE [num_frames, B].  pts_seq: DEVICE [n_rows, n_pts, 3]. */
int dyn_trajectory_points(const float* coeff, const float* basis, const float* pts, long n_pts, int B, const int* rows, int n_rows, int row_ref,
                          float* pts_seq, void* stream);

/* ---- a22 compute_optical_flow (render_ray.py:333-358): flows[v,r] = project_v(sum_s w[r,s] pts_seq[v,r,s]) - uv[r] ------------
 * proj: [V,16] from dyn_prepare_cameras (rows of K.inv(c2w)); flows: [V,R,2]. */
int dyn_render_flows(const float* weights, const float* pts_seq, const float* proj, const float* uv, int R, int S, int V, float* flows,
                     void* stream);
/* the same from the motion coefficients (the fused eval path: pts_seq [V,R,S,3] is never formed): pts [R,S,3], coeff [R,S,3 B], basis [frames,B],
 * rows_dev DEVICE [V] basis rows (negative: undisplaced), row_ref the reference time's row, B <= 16.  The expected point is formed through its linearity in the
 * coefficients (one pass over the samples for all views): equal to dyn_trajectory_points + dyn_render_flows up to the order of the fp32 sums (1e-7 relative) */
int dyn_render_flows_traj(const float* weights, const float* pts, const float* coeff, const float* basis, int B, const int* rows_dev, int row_ref,
                          const float* proj, const float* uv, int R, int S, int V, float* flows, void* stream);
/* ---- expected scene flow (render_ray.py:584-595 / :1086-1096): max(sum_s w (traj(row_p) - traj(row_ref)), sum_s w (traj(row_m) - traj(row_ref))) */
int dyn_expected_scene_flow(const float* weights, const float* coeff, const float* basis, int R, int S, int B, int row_p, int row_m, int row_ref,
                            float* exp_sf, void* stream);
/* ---- a2 RaySamplerSingleImage.get_rays_single_image (sample_ray.py:143-163): camera DEVICE [34]; rays_o, rays_d [(H/stride)*(W/stride),3] */
int dyn_image_rays(const float* camera, int H, int W, int render_stride, float* rays_o, float* rays_d, void* stream);

/* ---- helper exports of the reference's module surface (not on the render functions' own path, which fuses them) -------------------
 * sample_pdf (render_ray.py:19-64): bins [R,M+1], weights [R,M] (+1e-5 IN PLACE like the reference), u [R,N] or NULL (det) -> samples [R,N];
 * compute_ref_plucker_coordinate (:372-377): [R,6]; compute_src_plucker_coordinate (:380-396): pts [R,S,3] (per_view_pts = 0) or
 * [V,R,S,3] (per_view_pts = 1), cams [V,34] -> [R,S,V,6].  Both form the moment with torch.cross WITHOUT dim in the reference (:375, :392), which
 * crosses over the first axis of size 3 -- the views when V == 3, else the rays when R == 3, else the samples when S == 3, else xyz: these entry
 * points (and dyn_static_net / dyn_train_static_embed, which form the moments in their kernels) do the same, so R and S are separate arguments. */
int dyn_sample_pdf(const float* bins, float* weights, const float* u, int R, int M, int N, float* samples, void* stream);
int dyn_plucker_ref(const float* ray_o, const float* ray_d, int R, float* out, void* stream);
int dyn_plucker_src(const float* pts, int per_view_pts, const float* cams, int R, int S, int V, float* out, void* stream);
/* Projector.compute_projections (projection.py:32-59) and Projector.compute_angle (:61-101): xyz [V,n_pts,3] (+ xyz_st [V,n_pts,3], query_center [4] for
 * the angles), proj [V,16] from dyn_prepare_cameras -> pix [V,n_pts,2], in_front [V,n_pts] (0 / 1), ray_diff [V,n_pts,4]; either output group may be NULL. */
int dyn_project_points(const float* xyz, const float* xyz_st, const float* proj, const float* query_center, int V, long n_pts, float* pix,
                       float* in_front, float* ray_diff, void* stream);

/* ---- section 8(f)1: the 2-D feature encoder that feeds the path (feature_network.py:179-311, the executed part of ResNet.forward:
 * conv 7x7/2 -> InstanceNorm -> ReLU -> layer1 (3 BasicBlocks, reflect padding) -> 1x1 conv; 32 coarse + 32 fine channels at 1/4 resolution).
 * Channels-last throughout: images [N,H,W,3] as the data loader stores them, outputs [N,Hf,Wf,32] = the gather kernel's feat_cl layout.
 * dyn_encoder_pack: HOST pointers to the row-major fp32 tensors in this order (state-dict names of ibrnet.feature_network.ResNet):
 *   conv1.weight bn1.weight bn1.bias
 *   layer1.0.conv1.weight layer1.0.bn1.weight .bias layer1.0.conv2.weight layer1.0.bn2.weight .bias
 *   layer1.0.downsample.0.weight layer1.0.downsample.1.weight .bias
 *   layer1.1.conv1.weight layer1.1.bn1.weight .bias layer1.1.conv2.weight layer1.1.bn2.weight .bias
 *   layer1.2.conv1.weight layer1.2.bn1.weight .bias layer1.2.conv2.weight layer1.2.bn2.weight .bias
 *   out_conv.weight out_conv.bias */
size_t dyn_encoder_blob_floats(void);
int dyn_encoder_pack(const float* const* tensors, float* blob, size_t blob_floats);
size_t dyn_encoder_workspace_bytes(int N, int H, int W);
int dyn_encoder_out_size(int H, int W, int* Hf, int* Wf);
typedef struct {
  int N, H, W;              /* images */
  const float* blob;        /* DEVICE copy of the packed encoder */
  const float* images;      /* [N,H,W,3] */
  float* coarse;            /* [N,Hf,Wf,32]: channels 0..31 of out_conv (x_coarse) */
  float* fine;              /* [N,Hf,Wf,32]: channels 32..63 (x_fine) */
  void* workspace;
  size_t workspace_bytes;
} DynEncoderParams;
int dyn_encoder_forward(const DynEncoderParams* p, void* stream);

/* ---- training form of the encoder (autograd of ibrnet/feature_network.py:179-311; train.py:272-281 optimises feature_net): explicit
 * im2col + dyn_train_gemm for the convolutions, row kernels for what sits between; channels-last fp32 maps [N, H, W, C]. ----
 * dyn_enc_im2col: col[row, (ky * KW + kx) * C + c] = in[n, reflect(oy * stride - pad + ky), reflect(ox * stride - pad + kx), c],
 *   row = (n * Hout + oy) * Wout + ox (padding_mode='reflect' as conv3x3 / conv1 of the reference; pad 0 for the 1x1 convolutions); ldc a
 *   multiple of 4, columns KH * KW * C .. ldc - 1 are written as zeros;
 * dyn_enc_col2im: the adjoint, din += (a gather over the patches that contain a pixel; din holds whatever gradient the map already has);
 * dyn_enc_in_stats: stats[n][c] = {sum, sum of squares} over the HW pixels of image n (fp64, ZEROED by the caller), 64 channels;
 * dyn_enc_in_apply: y = [relu](InstanceNorm(x) * gamma + beta [+ res])  (nn.InstanceNorm2d(affine=True, eps=1e-5), BasicBlock.forward);
 * dyn_enc_in_bwd: its backward -- dyr = relu ? dy * (y > 0) : dy; dx = gamma * rstd * (dyr - mean(dyr) - xhat * mean(dyr * xhat));
 *   dres (may be NULL) = dyr (the residual branch); dgamma += sum dyr * xhat, dbeta += sum dyr; sums2 [N][64][2] doubles of workspace. */
int dyn_enc_im2col(const float* in, int N, int Hin, int Win, int C, int KH, int KW, int stride, int pad, int Hout, int Wout, float* col, long ldc,
                   void* stream);
int dyn_enc_col2im(const float* dcol, long ldc, int N, int Hin, int Win, int C, int KH, int KW, int stride, int pad, int Hout, int Wout, float* din,
                   void* stream);
int dyn_enc_in_stats(const float* x, int N, long HW, double* stats, void* stream);
int dyn_enc_in_apply(const float* x, const double* stats, const float* gamma, const float* beta, const float* res, int relu, int N, long HW, float* y,
                     void* stream);
int dyn_enc_in_bwd(const float* dy, const float* y, int relu, const float* x, const double* stats, const float* gamma, int N, long HW, double* sums2,
                   float* dx, float* dres, float* dgamma, float* dbeta, void* stream);

/* ---- how the network kernels of this build multiply (csrc/dyn_mlp.h): split terms = partial products kept per fp32 product (1, 3 or 6;
 * 0 = native fp32 MFMA engine); split kind = what the operand parts are: 0 none (fp32 MFMA), 1 bf16 (3 terms: 16 mantissa bits per
 * operand; 6 terms: fp32-class), 2 IEEE half (3 terms: 22 mantissa bits per operand, fp32-class; the shipped engine.  1 term: one half
 * per operand, the 11 significant bits of TF32 -- libdynibar_hip_x1.so, the `half` engine of dynibar_amd.engine) --------------- */
int dyn_mlp_split_terms(void);
int dyn_mlp_split_kind(void);

/* ---- self-test of the MFMA chain engine: y = elu(W elu(W x + b) + b), W [64,64], b [64] HOST; x, y [rows,64] DEVICE;
 * stream_buf: DEVICE scratch of 2 * 3 * 4096 floats ------------------------------------------------------------------- */
int dyn_mlp_selftest(const float* W, const float* b, const float* x, float* y, int rows, float* stream_buf, void* stream);

/* ---- per-kernel timing: when enabled, every kernel launched by this library is bracketed by HIP events on its launch stream.
 * dyn_profile_read synchronises the pending events, returns the summed milliseconds and launch counts per kernel slot
 * (dyn_profile_count() slots, named by dyn_profile_name) and resets the totals.  Not thread-safe; meant for bench.py. ------ */
int dyn_profile_enable(int on);
int dyn_profile_count(void);
const char* dyn_profile_name(int slot);
int dyn_profile_read(float* total_ms, int* launches);

/* ==== f3 (first slice): training of the static branch -- the reference's static bootstrap stage (train.py:116-199: loss on
 * ret['outputs_coarse_st']['rgb'], loss.backward() through raw2outputs_vanilla (render_ray.py:134-201), DynibarStatic.forward
 * (mlp_network.py:423-527) and Projector.compute's F.grid_sample (projection.py:160-167) into the module's parameters and the static
 * feature maps).  Replaces torch autograd for that graph.  The step is a sequence of the primitives below over row-major fp32
 * activation matrices kept in HBM (dynibar_amd/train_static.py holds the sequence); N = R S V rows (row = point * V + view),
 * P = R S points.  `ld*` are leading dimensions in floats, `*_stride` element strides of per-row scalars. =============================== */

/* C[M,N] (ldc) = epilogue(A . B): element (m,k) of A at A[m a_rs + k a_ks], element (k,n) of B at B[n b_rs + k b_ks] (one unit stride
 * each).  Forward of nn.Linear: A = X (a_ks = 1), B = W[N,K] (b_rs = ldw, b_ks = 1).  Data gradient dX = dZ W: A = dZ, B rows = input
 * features (b_rs = 1, b_ks = ldw).  Weight gradient dW = dZ^T X: A rows = output features (a_rs = 1, a_ks = ld_dz), B rows = input
 * features (b_rs = 1, b_ks = ldx), K = number of rows, k_split > 1 with accumulate = 2.
 * epilogue: + bias[n] + addend[(m / add_div) ld_add + n] (NULL to skip; with add_div = 1 the addend may be C itself -- C += A . B with plain
 * 16-byte stores, every element read and written by one thread), act (0 none, 1 ELU, 2 ReLU); accumulate 0 store, 1 or 2: += by fp32 atomics
 * (2 is required with k_split > 1).
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x16_f16: every operand split into two half parts (22 mantissa bits), 3 partial products; the
 * gradient operand A is first multiplied by the power of two that brings a_absmax to 2^14 (undone in the epilogue). */
typedef struct {
  const float* A;
  long a_rs, a_ks;
  const float* B;
  long b_rs, b_ks;
  float* C;
  long ldc;
  int M, N, K;
  const float* bias;
  const float* addend;
  long ld_add;
  int add_div;
  int act;
  int accumulate;
  int k_split;
  const float* a_absmax; /* DEVICE scalar: largest |A| when A is a gradient tensor (scaled into the half range), NULL for operands of order one */
  const float* act_y;    /* data gradient through the PRODUCING layer's activation: C = (A . B) * act'(act_y[m ld_y + n]) from that layer's saved
                          * OUTPUT (ELU' = y > 0 ? 1 : y + 1; ReLU' = y > 0): the autograd of nn.ELU / nn.ReLU fused into the Linear's backward
                          * (mlp_network.py:342-397, 587-603).  NULL to skip; needs accumulate = 0 */
  long ld_y;
  int act_y_kind;        /* 1 ELU, 2 ReLU */
  float* colsum_part;    /* [ceil(M / 128), ld_part]: a workgroup leaves the column sums of its 128-row result tile in row (tile index); every
                          * entry [tile, 0:N) is written, no initialisation needed -- the partial sums of the NEXT
                          * bias gradient: autograd of nn.Linear's bias, mlp_network.py:342-397) -- NULL to skip; needs accumulate = 0 and
                          * 16-byte-aligned result rows (N, ldc multiples of 4) */
  long ld_part;
  float* amax_part;      /* [ceil(M / 128) * ceil(N / 128)], all written: largest |result| per workgroup (required with colsum_part) */
  const float* rowscale; /* [M] or NULL: C = act(diag(rowscale) (A . B) + addend + bias) -- the forward of a Linear applied to x * s[row] (x * weight,
                          * x * vis: mlp_network.py:470, 474) without materialising the scaled input; not with a split reduction */
  const float* kscale;   /* [K] or NULL: B's element (n, k) is multiplied by kscale[k] -- the weight gradient dW = dZ^T (diag(s) X) of such a Linear
                          * from the unscaled X (the weight-gradient shape on the ring form only: both operands k-major with 16-byte-aligned rows, accumulate != 0) */
} DynTrainGemmParams;
int dyn_train_gemm(const DynTrainGemmParams* p, void* stream);
/* Developer / test knob: which kernel form dyn_train_gemm uses -- 0 automatic (default; the environment variable DYNIBAR_TRAIN_GEMM =
 * auto | tile | ring sets the initial value: the ring form for the backward products, the tile kernel for the forward ones), 1 the tile
 * kernel only, 2 the ring form wherever the operands allow it.  Results do not depend on it beyond the summation order. */
int dyn_train_gemm_mode(int mode);
/* second stage of colsum_part / amax_part: dbias[n] += sum over the tiles (dbias may be NULL), *absmax = max(*absmax, all of amax_part) */
int dyn_train_colsum_reduce(const float* colsum_part, long tiles, int N, long ld_part, float* dbias, const float* amax_part, long n_amax,
                            float* absmax, void* stream);

/* dZ = dY * act'(Y) in place (act 1: ELU, act 2: ReLU, both from the saved output Y; act 0: unchanged); dbias[c] += column sums (NULL to skip);
 * dseg[(row / seg), c] = sums over the seg rows of a point (gradient of a per-point addend; NULL to skip); absmax: see dyn_train_absmax. */
int dyn_train_act_bwd(float* dY, const float* Y, long rows, int cols, long ld_dy, long ld_y, int act, float* dbias, int seg, float* dseg,
                      long ld_seg, float* absmax, void* stream);
/* absmax[0] = max(absmax[0], largest |x|) over a [rows, cols] matrix: the scale of a gradient tensor for dyn_train_gemm's a_absmax (the
 * same by-product of dyn_train_act_bwd when `absmax` != NULL there); absmax is zeroed by the caller. */
int dyn_train_absmax(const float* x, long rows, int cols, long ld, float* absmax, void* stream);

/* mlp_network.py:423-448 + render_ray.py:372-396: a0 [N,104] = [PE(pts) 33 | PE(src Pluecker) 66 | ray_diff 4 | 0], ref_pe [R,68] =
 * [PE(ref Pluecker) 66 | 0 0], mask_eff [N] = mask (* (sum rgb > 1e-3) when mask_rgb).  centers: source camera centres, centers[v *
 * center_stride + 0..2] (proj + 12 with stride 16 from dyn_prepare_cameras). */
int dyn_train_static_embed(const float* pts, const float* ray_o, const float* ray_d, const float* centers, int center_stride,
                           const float* ray_diff, const float* rgb_feat, const float* mask, int R, int S, int V, int mask_rgb, float* a0,
                           float* ref_pe, float* mask_eff, void* stream);

/* mlp_network.py:450: f [N,72] = [rgb_feat 35 | src_feat * ref_feat[ray] 35 | 0 0]; backward: dsrc [N,.], dref [R,.] */
int dyn_train_build_f(const float* rgb_feat, const float* src_feat, long ld_src, const float* ref_feat, long ld_ref, long N, int rows_per_ray,
                      float* f, void* stream);
int dyn_train_build_f_bwd(const float* df, long ld_df, const float* src_feat, long ld_src, const float* ref_feat, long ld_ref, long R,
                          int rows_per_ray, float* dsrc, long ld_dsrc, float* dref, long ld_dref, void* stream);

/* pooling weights over the views of a point.  mode 0 (mlp_network.py:452-459): in = dot products (ray_diff + 3, stride 4), s_param =
 * the pooling temperature `s` (NULL: anti_alias_pooling = 0); mode 1 (:470-471,:476,:481): in = vis_fc2 logits; also writes vis, the mean
 * weight per point and the number of valid views.  backward: dw -> ds (mode 0, += one scalar) or dlogit (mode 1; dvis_direct and dwmean
 * are the other uses of vis and of the mean weight). */
int dyn_train_view_weights(int mode, const float* in, long in_stride, const float* mask, const float* s_param, long P, int V, float* w,
                           float* vis_out, long vis_stride, float* wmean, long wmean_stride, float* nvalid, void* stream);
int dyn_train_view_weights_bwd(int mode, const float* in, long in_stride, const float* mask, const float* s_param, long P, int V,
                               const float* w, const float* dw, const float* dvis_direct, long dvis_stride, const float* vis, long vis_stride,
                               const float* dwmean, long dwmean_stride, float* dlogit, long dlogit_stride, float* ds, void* stream);

/* fused_mean_variance (mlp_network.py:115-119) over the V rows of each point, C columns; backward into dx (accumulate 0/1) and dw. */
int dyn_train_meanvar(const float* x, long ldx, const float* w, long P, int V, int C, float* mean, float* var, long ld_out, void* stream);
int dyn_train_meanvar_bwd(const float* x, long ldx, const float* w, long P, int V, int C, const float* mean, const float* dmean,
                          const float* dvar, long ld_stat, float* dx, long ld_dx, int accumulate, float* dw, int dw_accumulate, void* stream);

/* y = x * s[row] (mlp_network.py:465,:469) and its backward */
int dyn_train_rowscale(const float* x, long ldx, const float* s, long s_stride, long N, int C, float* y, long ldy, void* stream);
int dyn_train_rowscale_bwd(const float* dy, long ld_dy, const float* x, long ldx, const float* s, long s_stride, long N, int C, float* dx,
                           long ld_dx, int accumulate, float* ds, long ds_stride, int ds_accumulate, void* stream);

/* mlp_network.py:466-468: x2 = x1 + xv[:, :128], vis0 = sigmoid(xv[:, 128]) mask; with ray_diff [N,4] != NULL the row of x2 is laid out as
 * rgb_fc.0's per-view input [x2 128 | vis (written later) | ray_diff 4 | 0 0 0] (ld2 >= 136, :495-503); backward fills dxv [N, 129] */
int dyn_train_vis_split(const float* x1, long ld1, const float* xv, long ldv, const float* mask, const float* ray_diff, long N, float* x2,
                        long ld2, float* vis0, void* stream);
int dyn_train_vis_split_bwd(const float* dx2, long ld_dx2, const float* dvis0, const float* xv, long ldv, const float* mask, long N, float* dxv,
                            long ld_dxv, void* stream);
/* The two calls above followed by dyn_train_act_bwd in ONE pass over the rows (128 columns, 16-byte-aligned rows):
 *  dyn_train_rowscale_act_bwd: dx = (dx + dy * s[row]) * act'(x), ds[row] (=|+=) <dy[row], x[row]> -- x is both what s multiplied in the
 *    forward pass and the saved output of the activation in front of it (mlp_network.py:466-470: x = base_fc(...); vis_fc(x * weight));
 *  dyn_train_vis_split_act_bwd: dxv[:, 0:128] = dx2 * ELU'(xv[:, 0:128]), dxv[:, 128] = dvis0 * mask * sigmoid'(xv[:, 128]) * ELU'(xv[:, 128])
 *    (mlp_network.py:470-473: vis_fc ends in an ELU over its 129 outputs); with dxs != NULL (then dvis0 may be NULL) the backward of
 *    vis_fc2's input x * vis (:474) comes first in the same pass: dx2 += dxs * vis0[row] (written back), dvis0[row] = <dxs[row], x2[row]>.
 * dbias (may be NULL) += the column sums of the result (128 / 129 entries), absmax (may be NULL) = max(absmax, largest |result|). */
int dyn_train_rowscale_act_bwd(const float* dy, long ld_dy, const float* x, long ldx, const float* s, long s_stride, long N, float* dx,
                               long ld_dx, float* ds, long ds_stride, int ds_accumulate, int act, float* dbias, float* absmax, void* stream);
int dyn_train_vis_split_act_bwd(float* dx2, long ld_dx2, const float* dvis0, const float* xv, long ldv, const float* mask, long N, float* dxv,
                                long ld_dxv, float* dbias, float* absmax, const float* dxs, long ld_dxs, const float* x2, long ldx2,
                                const float* vis0, void* stream);
/* Forward of a Linear with ONE output (mlp_network.py:474-476, 487-493, 505-507): y[row * y_stride] = <X[row, 0:C], w> + bias[0] (bias may be
 * NULL) for C = 4 * 2^k <= 256 columns in 16-byte-aligned rows; fp32 products and sums. */
int dyn_train_rowdot(const float* X, long ldx, const float* w, const float* bias, long N, int C, float* y, long y_stride, void* stream);
/* Data gradient of a Linear with ONE output through the activation in front of it (autograd of vis_fc2.2 / rgb_fc.4 / out_geometry_fc.2 and
 * of the ELU before them, mlp_network.py:474-476, 487-493, 505-507): dX[row, c] = dz[row] * w[c] * act'(Y[row, c]) for C = 4 * 2^k <= 256 columns
 * in 16-byte-aligned rows; dbias (may be NULL) += column sums, absmax (may be NULL) = max(absmax, largest |dX|); dW (may be NULL; needs
 * act != 0) [C] += sum over the rows of dz[row] * Y[row, :], the layer's own weight gradient (its input is Y), in the same pass. */
int dyn_train_outer_act_bwd(const float* dz, long dz_stride, const float* w, const float* Y, long ld_y, long N, int C, int act, float* dX,
                            long ld_dx, float* dbias, float* absmax, float* dW, void* stream);

/* ScaledDotProductAttention (mlp_network.py:13-31) for 4 heads of 32: qkv [P,384] = q | k | v, nvalid [P] = views that see the point
 * (query rows with nvalid <= 1 are masked, :24 and :486-488), out [P,128], prob [R,4,S,S] saved for the backward;
 * backward: dscore [R,4,S,S] scratch, dqkv [P,384]. */
int dyn_train_attn(const float* qkv, const float* nvalid, int R, int S, float* out, float* prob, void* stream);
int dyn_train_attn_bwd(const float* qkv, const float* nvalid, int R, int S, const float* prob, const float* dout, float* dscore, float* dqkv,
                       void* stream);

/* out = LayerNorm_128(a + b; eps 1e-6) gamma + beta (mlp_network.py:99-102); saves xhat [P,128], rstd [P]; backward: din (the gradient
 * of both a and b), dgamma / dbeta += */
int dyn_train_layernorm(const float* a, const float* b, const float* gamma, const float* beta, long P, float* out, float* xhat, float* rstd,
                        void* stream);
int dyn_train_layernorm_bwd(const float* dout, const float* xhat, const float* rstd, const float* gamma, long P, float* din, float* dgamma,
                            float* dbeta, void* stream);

/* mlp_network.py:503-527: masked softmax of the rgb_fc logits over views, rgb = sum_v rgb_in blend, sigma filled with -1e9 where no
 * view sees the point -> raw [P,4]; blend [N] saved.  backward: draw [P,4] -> dlogit [N], dsigma [P]. */
int dyn_train_blend(const float* logit, long logit_stride, const float* mask, const float* rgb_feat, const float* sigma, long sigma_stride,
                    const float* nvalid, long P, int V, float* blend, float* raw, void* stream);
int dyn_train_blend_bwd(const float* draw, const float* blend, const float* mask, const float* rgb_feat, const float* nvalid, long P, int V,
                        float* dlogit, long dlogit_stride, float* dsigma, long dsigma_stride, void* stream);

/* backward of raw2outputs_vanilla (render_ray.py:134-201): alpha, weights as saved by dyn_composite; drgb [R,3], ddepth [R],
 * dweights [R,S] (each may be NULL) -> draw [R,S,4].  S <= 4096.  The sums over the samples BEHIND a sample are formed directly, walking the ray from
 * its far end (not as total - prefix: far down a ray that difference is pure rounding, coherent along the ray). */
int dyn_train_composite_bwd(const float* raw, const float* z_vals, const float* alpha, const float* weights, const float* drgb,
                            const float* ddepth, const float* dweights, int R, int S, float* draw, void* stream);

/* backward of the bilinear feature gather (projection.py:160-167, F.grid_sample w.r.t. the maps): drgb_feat[row, col0 .. col0 + F)
 * scattered with the forward's taps into dfeat_cl [V,Hf,Wf,F] (channels-last, zeroed by the caller; atomic +=).  pts_st [R,S,3], or
 * xyz [V,R,S,3] != NULL: the per-view motion-displaced points of the dynamic branch. */
int dyn_gather_bwd(const float* pts_st, const float* xyz, const float* proj, int R, int S, int V, int Hf, int Wf, int F, float img_h, float img_w,
                   const float* drgb_feat, long ld_d, int col0, float* dfeat_cl, void* stream);

/* ==== f3, second slice: DynibarDynamic.forward (mlp_network.py:236-316) and the two-branch raw2outputs (render_ray.py:214-330) for
 * training: the dynamic net reuses the primitives above (dynibar_amd/train_dynamic.py holds its sequence) plus these. ================== */

/* y[row, c] = x[row, c] + tab[(row % period), c]: the time feature of mlp_network.py:244-249 on every row (period 1), the positional table
 * of :280 on every ray (period S).  The backward of both is the identity on x. */
int dyn_train_add_table(const float* x, long ldx, const float* tab, long ld_tab, int period, long rows, int C, float* y, long ldy, void* stream);

/* Fourier features of the dynamic net (mlp_network.py:147-160,:290,:303): pts_pe [P,36] = [PE_5(pts) 33 | 0 0 0], dir_pe [R,28] = [PE_4(dir) 27 | 0] */
int dyn_train_dynamic_embed(const float* pts, const float* ray_d, long P, int R, float* pts_pe, float* dir_pe, void* stream);

/* colour / density head (mlp_network.py:295-315): raw [P,4] = [sigmoid(logit) or 0 where no view sees the point | sigma - shift or -1e9] */
int dyn_train_dynamic_head(const float* logit, long ld_logit, const float* sigma, const float* nvalid, float shift, long P, float* raw, void* stream);
int dyn_train_dynamic_head_bwd(const float* draw, const float* raw, const float* nvalid, long P, float* dlogit, long ld_dlogit, float* dsigma,
                               void* stream);

/* backward of raw2outputs (render_ray.py:246-330): upstream gradients of rgb, rgb_static, rgb_dy [R,3], depth [R], weights_dy, weights_st,
 * weights [R,S] (each may be NULL) -> draw_dy, draw_st [R,S,4].  S <= 4096; suffix sums as in dyn_train_composite_bwd. */
int dyn_train_composite2_bwd(const float* raw_dy, const float* raw_st, const float* z_vals, const float* g_rgb, const float* g_rgb_st,
                             const float* g_rgb_dy, const float* g_depth, const float* g_wd, const float* g_ws, const float* g_w, int R, int S,
                             float* draw_dy, float* draw_st, void* stream);

/* ==== f3, third slice: the motion path of train.py:283-467 -- gradients w.r.t. the sample locations and through them into MotionMLP
 * (mlp_network.py:558-618; its Linear layers are dyn_train_gemm with act 2 = ReLU, dyn_train_act_bwd act 2) and the trajectory basis. ====== */

/* PeriodicEmbed (mlp_network.py:530-555) of x [rows, D] (ldx): out [rows, ld] = [x | cos(f_k x) k < n | sin(f_k x)]; freqs: HOST array of
 * n_freqs <= 16 frequencies.  backward w.r.t. x (accumulate 0/1). */
int dyn_train_embed(const float* x, long ldx, long rows, int D, const float* freqs, int n_freqs, float* out, long ld, void* stream);
int dyn_train_embed_bwd(const float* x, long ldx, long rows, int D, const float* freqs, int n_freqs, const float* dout, long ld, float* dx, long ld_dx,
                        int accumulate, void* stream);

/* x [R,S,C]: the last n_last samples of every ray zeroed, the rest multiplied by scale (render_ray.py:961,:1129 `raw_coeff[:, -n:, :] *= 0`,
 * mlp_network.py:618 `/ sf_mag_div`); applied to the gradient it is the backward of the same. */
int dyn_train_zero_tail(float* x, long R, int S, int C, int n_last, float scale, void* stream);

/* backward of dyn_trajectory_points (render_ray.py:361-369,:965-985): dseq [n_rows, n_pts, 3] -> dcoeff [n_pts, 3B] (=), dbasis [frames, B]
 * (atomic +=, zeroed by the caller), dpts [n_pts, 3] (= ; may be NULL) */
int dyn_trajectory_bwd(const float* dseq, const float* coeff, const float* basis, long n_pts, int B, const int* rows, int n_rows, int row_ref,
                       float* dcoeff, float* dbasis, float* dpts, void* stream);

/* backward of dyn_render_flows (render_ray.py:333-358): dflows [V,R,2] -> dweights [R,S] (=), dseq [V,R,S,3] (=) */
int dyn_render_flows_bwd(const float* dflows, const float* weights, const float* pts_seq, const float* proj, int R, int S, int V, float* dweights,
                         float* dseq, void* stream);

/* backward of the gather w.r.t. the sample locations (F.grid_sample w.r.t. its grid, normalize(), compute_projections: projection.py:32-59,
 * :134-167): drgb_feat [N, ld_d] (columns 0..2 colours, 3..3+F features) -> dxyz [V,R,S,3] (=).  pts_st / xyz as in dyn_gather_bwd. */
int dyn_gather_bwd_pts(const float* pts_st, const float* xyz, const float* proj, const float* src_rgb, const float* feat_cl, int R, int S, int V,
                       int H, int W, int Hf, int Wf, int F, float img_h, float img_w, const float* drgb_feat, long ld_d, float* dxyz, void* stream);

/* ====== multi-GPU pixel gather (the counterpart of nn.DataParallel's gather of the rendered outputs, reference
 * ibrnet/model.py:134-159, around the chunk loop of render_image.py:60-217) ============================================================
 * Rays shard across ranks as contiguous tiles with no data-path collective; the one exchange of a frame is an all-gather of every rank's
 * packed [rows_per_rank, cols] fp32 pixel rows (rgb, depth, mask ...) over RCCL / xGMI.  `comm` is an ncclComm_t: the caller's own, or one made
 * by dyn_comm_init_rank.  RCCL is taken from the process image at run time (a PyTorch host has loaded its own librccl; a communicator is
 * only valid in the library instance that made it), else from librccl.so / $DYNIBAR_RCCL_LIB; without it these calls return DYN_E_INVALID. */
int dyn_comm_available(void);
/* id128: HOST buffer of 128 bytes (ncclUniqueId).  Rank 0 makes it, the host's own channel hands it to every rank. */
int dyn_comm_unique_id(void* id128);
int dyn_comm_init_rank(void** comm, int nranks, const void* id128, int rank);
int dyn_comm_size_rank(void* comm, int* nranks, int* rank);
int dyn_comm_destroy(void* comm);
/* recv [nranks, rows_per_rank, cols] <- send [rows_per_rank, cols] of every rank, in rank order, on `stream` (one equal-count ncclAllGather;
 * tiles are padded to the common size by the caller: balanced tiles differ by at most one ray). */
int dyn_gather_tiles(const float* send, float* recv, long rows_per_rank, int cols, void* comm, void* stream);

/* ====== virtual source views of the monocular path (render_source_vv.py, the producer of source_virtual_views_WxH/NNNNN/KK.png and
 * source_vv_poses.npy that ibrnet/data_loaders/monocular.py:312-325, 374-387 load) =====================================================
 * The splat of the third-party `splatting` package (render_source_vv.py:12, 58): source pixel (x, y) of batch entry b lands at
 * (X, Y) = (x + flow[b,0,y,x], y + flow[b,1,y,x]) and adds w * value to its four bilinear corners nw, ne, sw, se (corner 0..3; weights
 * (x0+1-X)(y0+1-Y), (X-x0)(y0+1-Y), (x0+1-X)(Y-y0), (X-x0)(Y-y0) with x0 = floor(X), y0 = floor(Y)); corners off the image, and
 * non-finite targets, contribute nothing.  Every output pixel is summed SEQUENTIALLY in ascending contribution id 4 (y W + x) + corner,
 * starting at +0.0, so the result is bitwise reproducible (no float atomics: a stable radix sort builds the inverted index).
 * Workspace: DEVICE scratch of dyn_splat_workspace_bytes(B,H,W) bytes (0: unsupported shape, B*H*W > 2^28), shared by both entries. */
size_t dyn_splat_workspace_bytes(int B, int H, int W);
typedef struct {
  int B, C, H, W;
  const float* frame;        /* [B,C,H,W] */
  const float* flow;         /* [B,2,H,W] */
  const float* multiplier;   /* [B,H,W] or NULL: contributions are w * (frame * multiplier) (the package's linear / softmax forms) */
  int normalize;             /* 0: summation.  1: out = num / (den + eps), den = the splatted multiplier (1 where multiplier is NULL) */
  float eps;                 /* the package's eps (1e-7) */
  float* out;                /* [B,C,H,W] */
  void* workspace;
  size_t workspace_bytes;
} DynSplatParams;
int dyn_splat(const DynSplatParams* p, void* stream);

/* render_forward_splat (render_source_vv.py:15-66) fused: P = depth K_src^-1 [x y 1], Q = K_dst (R P + t), flow = Q.xy / max(Q.z, 1e-8)
 * - (x, y), importance = 1 / Q.z, w = (importance - min_b) / (max_b - min_b + 1e-6) * 20 - 10 (per batch entry), then the softmax splat of
 * [src | importance | 1] with multiplier exp(w).  The probes (NULL to skip) receive the intermediate values the kernels actually used. */
typedef struct {
  int B, H, W, C;
  const float* src;          /* [B,H,W,C] channels-last, as the reference passes it */
  const float* depth;        /* [B,H,W] */
  const float* k_src_inv;    /* [B,3,3] */
  const float* rot;          /* [B,3,3] */
  const float* k_dst;        /* [B,3,3] */
  const float* t;            /* [B,3] */
  float eps;                 /* the package's eps (1e-7) */
  float* feat;               /* [B,C,H,W] warp_feature */
  float* disp;               /* [B,1,H,W] warp_disp */
  float* mask;               /* [B,1,H,W] or NULL: the splatted ones channel (the reference's commented-out warp_mask, :64) */
  float* flow;               /* probe [B,2,H,W] or NULL */
  float* importance;         /* probe [B,H,W] or NULL */
  float* weight_exp;         /* probe [B,H,W] or NULL: exp(w) */
  void* workspace;
  size_t workspace_bytes;
} DynForwardSplatParams;
int dyn_forward_splat(const DynForwardSplatParams* p, void* stream);

/* sobel_fg_alpha (render_source_vv.py:118-128): x [B,1,H,W] -> alpha [B,1,H,W] = exp(-beta |sobel(x)|), kornia spatial_gradient
 * (mode='sobel', normalized=False) with replicate padding */
int dyn_sobel_alpha(const float* x, int B, int H, int W, float beta, float* alpha, void* stream);

/* the per-view epilogue of render_source_vv.py:313-330: feat [B,C,H,W] (C >= 4: rgb in 0..255, alpha) -> out [B,H,W,3] uint8 =
 * uint8(255 clip(clip(rgb / 255, 0, 1) m, 0, 1)), m = erosion(clip(alpha, 0, 1) > 0.5, disk(1)); out-of-image neighbours do not erode */
int dyn_vv_finish(const float* feat, int B, int C, int H, int W, uint8_t* out, void* stream);

/* The virtual views of F frames x V views in one pass (render_source_vv.py:283-330 for every frame): per frame f
 *   x = (1 / disp[f]) / 10, alpha = exp(-0.5 |sobel(x)|) as dyn_sobel_alpha, source = (255 img[f], alpha), depth = 1 / disp[f];
 * per view b = f * V + v the forward splat of dyn_forward_splat with k_src_inv = k_inv[f], k_dst = k[f], rot[b], t[b] and the importance
 * minimum / maximum of view b; then dyn_vv_finish.  Every value is formed by the operations of those three entries in their order and every
 * sum runs in ascending contribution id, so out is BIT-IDENTICAL to sobel -> forward splat of the frame repeated V times -> finish; no frame
 * is repeated in memory (view b reads frame b / V) and the splatted channels nothing reads (importance, ones) are not formed.
 * tenth_by_division: x = depth / 10.f; 0: x = depth * (1.f / 10.f), which is what torch evaluates for `depth / 10.0` on a HIP tensor (a
 * division by a host scalar becomes a multiplication by its fp32 reciprocal there), so 0 reproduces the script on a HIP device and 1 on a
 * host tensor.  k_inv is the caller's inverse of k, as dyn_forward_splat takes it.  View b is written to out + b * out_pitch (BYTES),
 * [H,W,3] contiguous; bytes between views are not written.  No host synchronisation, no device-to-host copy, nothing allocated.
 * Workspace: DEVICE scratch of dyn_vv_frames_workspace_bytes(F,V,H,W) bytes on 16 bytes (0: unsupported: a size below 1, V > 65535 or
 * F*V*H*W > 2^28).  Frames are sorted in groups that need no more radix passes than one frame's views; the grouping does not change a bit. */
size_t dyn_vv_frames_workspace_bytes(int F, int V, int H, int W);
typedef struct {
  int F, V, H, W;
  const float* img;          /* [F,H,W,3] in 0..1 */
  const float* disp;         /* [F,H,W] */
  const float* k;            /* [F,3,3] source = destination intrinsics */
  const float* k_inv;        /* [F,3,3] */
  const float* rot;          /* [F*V,3,3] */
  const float* t;            /* [F*V,3] */
  float eps;                 /* the package's eps (1e-7) */
  int tenth_by_division;
  uint8_t* out;
  int64_t out_pitch;
  void* workspace;
  size_t workspace_bytes;
} DynVvFramesParams;
int dyn_vv_frames(const DynVvFramesParams* p, void* stream);

/* ====== the training objective of the monocular main loop (train.py:300-456) on the dictionary render_rays_mono(is_train=True) returns =====
 * Forward: k_objective_rays (one wavefront per ray: the Charbonnier colour terms, disparity, flow, sum_S weights_dy / weights_st -> ratio ->
 * entropy and the static mask, the distortion loss by two wave scans) and k_objective_samples (one thread per sample: consistency and the
 * three scene-flow regularisers) store per-workgroup partial sums (double, plain stores, every entry written); k_objective_finish adds them in
 * a fixed order and forms the nine logged scalars.  No float atomics anywhere: two calls on the same inputs give the same bits.
 * Backward: element-wise given the forward's sums (k_objective_rays_bwd, k_objective_samples_bwd); grad_loss is read from device memory.
 * Conventions as torch has them: sign(0) = 0, clamp(min=c) passes the gradient where x >= c.  Everything the reference detaches
 * (occ_weights, occ_weight_map, the static mask's 1 - ratio factor and its < 0.1 mask) receives no gradient.
 * Per-ray and per-sample arithmetic is double: the result is the float64 value of the formulas on the fp32 inputs, rounded once.
 * Workspace: DEVICE scratch of dyn_objective_workspace_bytes(R, S) bytes (0: unsupported shape); the backward reads what the forward left. */
#define DYN_OBJECTIVE_LOGGED 9  /* loss, rgb, cycle, flow, disp, reg, entropy, distortion, static */
size_t dyn_objective_workspace_bytes(int R, int S);
typedef struct {
  int R, S;                  /* rays, samples per ray (S >= 2) */
  int T;                     /* frames of pts_traj_* (0: no consistency term) */
  int NV;                    /* flow views, 0..6 */
  /* supervision (ray_batch) */
  const float *t_rgb;        /* [R,3] */
  const float *t_disp;       /* [R] */
  const float *t_flows;      /* [>=NV,R,2] */
  const float *t_masks;      /* [>=NV,R,1] */
  const float *motion_mask, *static_mask;  /* [R] */
  /* outputs_coarse_ref */
  const float *rgb_ref, *rgb_dy, *rgb_static;  /* [R,3] */
  const float *depth;        /* [R] */
  const float *render_flows; /* [NV,R,2] */
  const float *weights, *weights_dy, *weights_st, *s_vals;  /* [R,S] */
  const uint8_t *mask_ref;   /* [R] (torch.bool) */
  /* outputs_coarse_ref_dy, outputs_coarse_anchor, outputs_coarse_anchor_dy */
  const float *rgb_ref_dy, *rgb_anc, *rgb_anc_dy;  /* [R,3] */
  const float *owm_anc, *owm_anc_dy;  /* [R] occ_weight_map */
  const uint8_t *mask_ref_dy, *mask_anc, *mask_anc_dy;  /* [R] */
  const float *pts_traj_ref, *pts_traj_anchor;  /* [T,R,S,3], NULL: the consistency term is not evaluated */
  const float *occ_weights;  /* [R,S] */
  const float *sf_seq;       /* [6,R,S,3], NULL: the scene-flow regularisers are not evaluated */
  /* weights of the terms with the schedule applied (0: the term is left out and logs 0) */
  double k_rgb;              /* Criterion(ref) + temporal(anchor) */
  double k_rgb_dyn;          /* the dynamic-only term: 1 while epoch < init_decay_epoch */
  double k_rgb_dy;           /* the two _dy terms: 10 ** -divisor */
  double w_disp, w_flow, w_cycle, w_reg, w_entropy, w_distortion;
  double k_static;           /* the adaptive static term */
  double k_static2;          /* its divisor > 4 addition: 0.1 */
  void* workspace;
  size_t workspace_bytes;
} DynObjectiveParams;
/* loss [1], logged [DYN_OBJECTIVE_LOGGED]: device floats */
int dyn_objective_fwd(const DynObjectiveParams* p, float* loss, float* logged, void* stream);
typedef struct {             /* cotangents; NULL: not wanted, not computed.  Every element of a non-NULL tensor is written once. */
  const float* grad_loss;    /* [1] device */
  float *rgb_ref, *rgb_dy, *rgb_static, *rgb_ref_dy, *rgb_anc, *rgb_anc_dy, *depth, *render_flows, *weights, *weights_dy, *weights_st;
  float *pts_traj_ref, *pts_traj_anchor, *sf_seq;
} DynObjectiveGrads;
int dyn_objective_bwd(const DynObjectiveParams* p, const DynObjectiveGrads* g, void* stream);

/* eff_distloss_native of torch_efficient_distloss (the O(S) form of the mip-NeRF-360 distortion loss): per ray
 * (1/3) sum_i interval_i w_i^2 + 2 sum_{i>=1} (w_i m_i sum_{j<i} w_j - w_i sum_{j<i} w_j m_j), then the mean over the R rays.
 * w, m, interval: [R,S] rows of stride ld_* floats (unit stride along S).  partial: DEVICE scratch of dyn_distloss_partials(R) doubles. */
long dyn_distloss_partials(long R);
int dyn_distloss_fwd(const float* w, long ld_w, const float* m, long ld_m, const float* interval, long ld_i, long R, int S, double* partial,
                     float* loss, void* stream);
/* dw / dm / dinterval [R,S] contiguous, NULL: not wanted */
int dyn_distloss_bwd(const float* w, long ld_w, const float* m, long ld_m, const float* interval, long ld_i, long R, int S, const float* grad_loss,
                     float* dw, float* dm, float* dinterval, void* stream);

/* ====== frame metrics of the evaluation loop (eval_nvidia.py:201-247 calculate_psnr / calculate_ssim, :383-457 without LPIPS) ==============
 * One call evaluates M masks (1..8) on one frame.  Preparation (:383-396): valid = ((r + g) + b > 1e-3f) per pixel of pred, in fp32 in
 * numpy's order of addition; a uint8 target is float(u8) / 255.0f; with apply_valid both images are multiplied by valid -- all bit-exact
 * against numpy.  The SSIM map is skimage.metrics.structural_similarity's as :242-244 calls it (7 x 7 uniform window, scipy's `reflect`
 * boundary, sample covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2, per channel, not cropped) with R = data_range.  Window sums, variances, S
 * and the masked sums are double, accumulated in a fixed order: k_metrics_tile stores one row of partial sums per tile of 32 x 8 pixels
 * (plain stores, every entry written), k_metrics_finish adds the rows in a fixed order.  No float atomics: two calls give the same bits,
 * and a mask's sums do not depend on the other masks of the call.
 * sums [M][3] (DEVICE doubles): sum((a - b)^2 m), sum(S m), sum(m) over [H,W,3], a / b the prepared pred / target.
 * Workspace: DEVICE scratch of dyn_frame_metrics_workspace_bytes(H, W, M) bytes, 8-byte aligned (0: unsupported shape -- H or W below 7,
 * H*W*3 >= 2^31, M outside 1..8). */
size_t dyn_frame_metrics_workspace_bytes(int H, int W, int M);
typedef struct {
  int H, W;
  int M;                     /* masks evaluated (1..8), the valid mask included when valid_as_mask0 is set */
  const float* pred;         /* [H,W,3] */
  const void* target;        /* [H,W,3] fp32, or uint8 when target_is_u8 is set */
  int target_is_u8;
  const float* masks;        /* M - valid_as_mask0 masks of fp32 weights (not necessarily 0 / 1); NULL when there is none */
  long mask_stride;          /* floats from one mask to the next */
  int mask_channels;         /* 3: [H,W,3]; 1: [H,W], the weight of a pixel applies to its three channels */
  int apply_valid;           /* multiply both images by valid (:395-396) */
  int valid_as_mask0;        /* mask 0 is valid itself (the whole-frame numbers of the script, :398) */
  double data_range;         /* R > 0, finite */
  double* ssim_map;          /* [H,W,3] or NULL */
  uint8_t* valid;            /* [H,W] 0 / 1 or NULL */
  float* pred_out;           /* [H,W,3] or NULL: the prepared images */
  float* target_out;
  void* workspace;
  size_t workspace_bytes;
} DynFrameMetricsParams;
int dyn_frame_metrics(const DynFrameMetricsParams* p, double* sums, void* stream);

/* ====== masked LPIPS of the evaluation loop (eval_nvidia.py:250-263 im2tensor, :289-291, :402-457): LPIPS v0.1, net 'alex', 'net-lin' ========
 * One call evaluates M masks (1..8) on one frame; the features are computed once for all of them.
 *   1. Preparation as dyn_frame_metrics (valid, float(u8) / 255.0f, both images times valid with apply_valid), then x / 0.5f - 1.0f and the
 *      scaling layer (x - shift) / scale, shift (-.030, -.088, -.188), scale (.458, .448, .450): fp32, bit-exact against numpy.
 *   2. torchvision's AlexNet `features` (zero padding, bias), tapped after each ReLU: conv 3->64 k11 s4 p2 | max-pool 3 s2, conv 64->192 k5 p2 |
 *      max-pool 3 s2, conv 192->384 k3 p1 | conv 384->256 k3 p1 | conv 256->256 k3 p1.  fp32 products on the matrix pipe, fp32 accumulate.
 *   3. Per tap pixel n = f / (sqrt(sum_c f^2) + 1e-10), d_l = sum_c lin_l[c] (n0 - n1)^2, in double.
 *   4. A mask's channel 0 is resized to each tap by nearest neighbour, src = (dst * n_in) / n_out in integers; S_l = sum d_l m_l, M_l = sum m_l,
 *      double, fixed order.  lpips = sum_l S_l / M_l is formed by the caller (a tap with M_l = 0 contributes 0).
 *      NOT VERIFIED: the script's `models` package (NSFF's modified LPIPS) and its masked form were not available; this is the stated form.
 * No atomics: two calls give the same bits, a mask's sums do not depend on the other masks, identical images give exactly 0.
 * dyn_lpips_pack: HOST pointers to 15 row-major fp32 tensors: features.{0,3,6,8,10}.{weight,bias} of torchvision's alexnet in that order
 * (weight, bias, weight, ...), then lin0..lin4 ([64], [192], [384], [256], [256]).  Refused: a NULL tensor, a non-finite element, a negative
 * lin weight.  blob: HOST, dyn_lpips_blob_floats() floats; upload it 16-byte aligned.
 * sums [M][5][2] (DEVICE doubles): (S_l, M_l) per mask and tap.  maps (optional, DEVICE): the five d_l maps one after the other,
 * dyn_lpips_map_doubles(H, W) doubles, tap l being [H_l][W_l] with H_0 = (H - 7) / 4 + 1, H_1 = (H_0 - 3) / 2 + 1, H_2..4 = (H_1 - 3) / 2 + 1.
 * prepared (optional, DEVICE): [2][H][W][3] fp32, the prepared and scaled pred and target.
 * Workspace: DEVICE scratch of dyn_lpips_workspace_bytes(H, W, M) bytes, 16-byte aligned (0: unsupported shape -- H or W below 31, the
 * smallest image for which both max-pools have a full window, H*W*4 >= 2^31, M outside 1..8). */
size_t dyn_lpips_blob_floats(void);
int dyn_lpips_pack(const float* const* tensors, float* blob, size_t blob_floats);
size_t dyn_lpips_workspace_bytes(int H, int W, int M);
long dyn_lpips_map_doubles(int H, int W);
typedef struct {
  int H, W;
  int M;                     /* masks evaluated (1..8), the valid mask included when valid_as_mask0 is set */
  const float* blob;         /* DEVICE copy of the packed weights */
  const float* pred;         /* [H,W,3] */
  const void* target;        /* [H,W,3] fp32, or uint8 when target_is_u8 is set */
  int target_is_u8;
  const float* masks;        /* M - valid_as_mask0 masks of fp32 weights; channel 0 is used; NULL when there is none */
  long mask_stride;          /* floats from one mask to the next */
  int mask_channels;         /* 3: [H,W,3]; 1: [H,W] */
  int apply_valid;           /* multiply both images by valid */
  int valid_as_mask0;        /* mask 0 is valid itself */
  double* maps;              /* dyn_lpips_map_doubles(H, W) doubles or NULL */
  float* prepared;           /* [2][H][W][3] or NULL */
  void* workspace;
  size_t workspace_bytes;
} DynLpipsParams;
int dyn_lpips_frame(const DynLpipsParams* p, double* sums, void* stream);

/* ====== training batches from a device-resident scene (ibrnet/data_loaders/monocular.py:120-144, :300-425; sample_ray.py:262-331) ==========
 * The scene is uploaded once: frames and virtual views as uint8 images, every image padded to image_stride bytes (a multiple of 16, so
 * that dword loads stay aligned when H*W*3 is not a multiple of 4), the optional source masks as uint8 in the same way, disparity and
 * flows as fp32, the per-pixel masks as uint8 0 / 1.  A batch is then two launches:
 *   dyn_scene_views        the three source-view lists (ref, anchor, static; V = V_ref + V_anchor + V_static views, consecutive in desc,
 *                          images and cameras).  desc holds four int32 per view: image frame, virtual index (0..7) or -1, mask frame or -1,
 *                          intrinsics frame.  The pose is poses[image frame], or vposes[image frame][virtual index] for a virtual view.
 *                          images [V,H,W,3] = float(u8) / 255.0f, with a mask times float(m) / 255.0f (a one-channel mask applies to the
 *                          pixel's three channels) -- IEEE divisions: numpy's astype(float32) / 255.0 and src_rgb * st_mask bit for bit.
 *                          cameras [V,34] = [H, W, K(16), c2w(16)].
 *   dyn_scene_supervision  for R pixel indices sel[r] (row-major, y * W + x) of one frame: ray_o / ray_d [R,3] with the bits dyn_image_rays
 *                          gives those pixels, uv [R,2] = (x, y), rgb [R,3] by the same / 255.0f rule, and copies: disp [R], motion_mask
 *                          [R], static_mask [R], flows [6,R,2], masks [6,R].  sel NULL: every pixel in order (R must be H*W).
 *                          camera / anchor_camera [34] (each may be NULL): the cameras of frame and anchor_frame.
 * Every output element is written.  Limits: H*W*3 < 2^31; at most 32 views per list (the network engine's own limit) and at least one
 * in all; R >= 1.
 * Argument checking happens on the host BEFORE anything is launched: desc_host / sel_host are host-readable copies of the DEVICE arrays
 * desc / sel (the pinned staging buffer they were copied from), and a frame id, virtual index, mask frame or pixel index out of range, a
 * list of more than 32 views, or a virtual view / mask asked of a store that has none returns DYN_E_INVALID with a message.  The kernels
 * check the same indices again and write zeros for a bad one: they never read out of bounds. */
typedef struct {
  int N, H, W;                 /* frames, image size */
  long image_stride;           /* bytes from one stored image to the next: >= H*W*3, a multiple of 16 */
  const uint8_t* frames;       /* N images, 16-byte aligned */
  const uint8_t* vviews;       /* N*8 images (frame-major), or NULL */
  const uint8_t* src_masks;    /* N masks, or NULL */
  int mask_channels;           /* 1: [H,W]; 3: [H,W,3] */
  long mask_stride;            /* bytes from one mask to the next: >= H*W*mask_channels, a multiple of 16 */
  const float* intrinsics;     /* [N,16] */
  const float* poses;          /* [N,16] camera-to-world */
  const float* vposes;         /* [N,8,16], or NULL */
  const float* disp;           /* [N,H,W]      (the rest: dyn_scene_supervision only) */
  const uint8_t* motion_mask;  /* [N,H,W] 0 / 1 */
  const uint8_t* static_mask;  /* [N,H,W] 0 / 1 */
  const float* flows;          /* [N,6,H,W,2], 8-byte aligned */
  const uint8_t* flow_masks;   /* [N,6,H,W] 0 / 1 */
} DynSceneStore;
int dyn_scene_views(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_ref, int V_anchor, int V_static, float* images,
                    float* cameras, void* stream);
typedef struct {
  int frame, anchor_frame;
  int R;
  const int32_t* sel_host;     /* HOST copy of sel, read by the argument check */
  const int32_t* sel;          /* DEVICE [R], or NULL for all H*W pixels */
  float* ray_o;
  float* ray_d;
  float* uv;
  float* rgb;
  float* disp;
  float* motion_mask;
  float* static_mask;
  float* flows;                /* [6,R,2], 8-byte aligned */
  float* masks;                /* [6,R] */
  float* camera;               /* [34] or NULL */
  float* anchor_camera;        /* [34] or NULL */
} DynSceneSupervisionParams;
int dyn_scene_supervision(const DynSceneStore* s, const DynSceneSupervisionParams* p, void* stream);

/* ====== bullet-time frames from the same resident scene (render_monocular_bt.py:96-259 the item, :342-361 the output stage) ==================
 *   dyn_scene_views_target  dyn_scene_views for a frame rendered from a camera that is not one of the scene's: a view whose intrinsics
 *                           frame is -1 takes K from target_camera[2..17] (the script gives a virtual view the RENDER camera's intrinsics,
 *                           :195-199).  target_camera is a DEVICE [34] array [H, W, K(16), c2w(16)], target_camera_host its host copy for
 *                           the argument check (H and W must be the store's, every entry finite).  Both NULL: -1 is refused, DYN_E_INVALID,
 *                           like by dyn_scene_views itself, whose behaviour and output bits are unchanged.  The frame's own image, where a
 *                           ground truth is wanted, is one more view of the launch; its rays are dyn_image_rays on target_camera.
 *   dyn_frame_pack_u8       K images (1..4) of fp32 [H,W,3] -> out uint8 [K, H - 2 crop_h, (W - 2 crop_w) * (2 with gt_frame >= 0, else 1), 3]:
 *                           byte = (uint8)(255.0f * clip(x, 0, 1)), an fp32 multiply and a truncation -- numpy's
 *                           (255 * np.clip(x, 0, 1)).astype(np.uint8); NaN gives 0 (numpy's cast of NaN is platform-dependent), -inf,
 *                           negatives and -0.0 give 0, +inf and x > 1 give 255.  With gt_frame >= 0 the LEFT half of every output row is
 *                           the cropped row of frames + gt_frame * image_stride, copied (the store's bytes are what
 *                           255 * (float(b) / 255.0f) truncates to, for all 256 values).  Every output byte is written.
 *                           Refused: K outside 1..4, crops that leave no pixel, a null image or out, H*W*3 >= 2^31, out not on 4 bytes,
 *                           gt_frame outside -1..N-1 or without frames. */
int dyn_scene_views_target(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_ref, int V_anchor, int V_static,
                           const float* target_camera_host, const float* target_camera, float* images, float* cameras, void* stream);
typedef struct {
  int K, H, W;
  int crop_h, crop_w;          /* rows / columns dropped at each side */
  const float* image0;         /* K images [H,W,3]; the rest NULL */
  const float* image1;
  const float* image2;
  const float* image3;
  int gt_frame;                /* -1: none */
  int N;                       /* frames of the store (gt_frame >= 0) */
  const uint8_t* frames;       /* the store's frames and their stride (DynSceneStore), or NULL */
  long image_stride;
  uint8_t* out;                /* 4-byte aligned */
} DynFramePackParams;
int dyn_frame_pack_u8(const DynFramePackParams* p, void* stream);

/* ====== a time step of the multi-camera benchmark evaluation from the same resident scene (eval_nvidia.py:121-198, :350-354, :423-444) ======
 *   dyn_scene_views_masked  the two source-view lists of a TIME STEP (they do not depend on the target camera) in one launch: desc holds
 *                           V_src + V_static rows of four int32 as for dyn_scene_views (image frame, -1, mask frame or -1, intrinsics frame);
 *                           only a static view may name a mask frame, and the store's masks must then be one-channel [H,W] (the script's
 *                           coarse mask).  src_rgbs [V_src,H,W,3] and static_rgbs [V_static,H,W,3] = float(u8) / 255.0f; static_masks
 *                           [V_static,H,W] = float(m) / 255.0f, or exactly 1.0f for a mask frame of -1; with want_masked = 1 static_masked
 *                           [V_static,H,W,3] = static_rgbs * static_masks, one fp32 multiply per value (:350-354); with want_masked = 0
 *                           static_masked must be NULL and nothing is written for it.  src_cameras / static_cameras [.,34].  Each image
 *                           and mask is fetched once for all of its outputs; every output element is written.
 *                           Refused before a launch, DYN_E_INVALID: V_src or V_static outside 1..32, a required output that is NULL
 *                           (static_masked with want_masked), an index out of range, a virtual index other than -1, a mask frame on a
 *                           temporal view or without a mask store, a three-channel mask store.  The kernel checks the indices again.
 *   dyn_eval_mask_pair      mask: a stored 0 / 1 mask, uint8 [H,W,C] (C = 1 or 3), 4-byte aligned -> out fp32 [2,H,W,C] = (m, 1.0f - m),
 *                           m = float(byte), 16-byte aligned: the user masks dyn_frame_metrics takes for the script's dynamic and static
 *                           numbers (:423-444).  Every output element is written. */
int dyn_scene_views_masked(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_src, int V_static, int want_masked,
                           float* src_rgbs, float* src_cameras, float* static_rgbs, float* static_cameras, float* static_masks,
                           float* static_masked, void* stream);
int dyn_eval_mask_pair(const uint8_t* mask, int H, int W, int C, float* out, void* stream);

/* ====== the view panels the training loop logs (train.py:576-762 log_view_to_tb; utils.py:97-170 colorize; flow_utils.py:17-153) ============
 * Three launches turn the device-resident groups of a rendered frame into the values the script hands to its summary writer; nothing
 * goes through the host in between.  All images are H x W, n = H*W, H*W*3 < 2^31.  Inputs are never written (the script's flow_to_image
 * zeroes unknown pixels in its argument; these do not).  Inputs must be finite.
 *   dyn_viewlog_ranges    for K scalar images (1..4): ranges [K][2] (DEVICE doubles) = (vmin, vmax) of colorize without mask or range,
 *                         np.percentile(x, (1, 99)) by the `linear` method in numpy's arithmetic, vmax += 1e-6.  Image k is image[k], fp32
 *                         [H,W], or with magnitude[k] set it is formed from image[k] as fp32 [H,W,3] by sqrtf(fmaf(z, z, fmaf(y, y, x * x)))
 *                         -- torch.norm(dim=-1) on the host, bit for bit -- and also written to mag_out[k], fp32 [H,W] (required then).
 *                         The host passes what depends on n alone: rank[4] = the indices (0..n-1) of the order statistics below and
 *                         above the 1st and the 99th percentile, weight[2] = numpy's interpolation weights (doubles).  Per percentile
 *                         a, b = the two order statistics, d = fp32(b - a), then a + d t in double, or b - d (1 - t) where t >= 0.5.
 *                         One workgroup per image selects the four order statistics exactly: a radix select in three passes of 11 / 11 /
 *                         10 bits over the order-preserving integer key of the float (-0.0 counts as +0.0), integer LDS histograms only.
 *   dyn_viewlog_flow_max  for F flow images (1..12), fp32 [H,W,2]: maxrad [F] (DEVICE fp32) = max(-1, max sqrtf(u*u + v*v)) in fp32 over
 *                         the pixels, a pixel with |u| > 200 or |v| > 200 counting as (0, 0).  An integer maximum of the bits of
 *                         non-negative floats: independent of the order.
 *   dyn_viewlog_panels    one grid over every output element.
 *                         rgb panels (0..8): fp32 [H,W,3] -> fp32 [3,H,W], with rgb_clamp[i] clamped to 0..1 (torch.clamp).
 *                         map panels (0..4): x fp32 [H,W] and its (vmin, vmax) from ranges -> double [3,H,W] (map_chw) or [H,W,3]: in
 *                         double, clip(x, vmin, vmax), (x - vmin) / (vmax - vmin), clip(0, 1), index min(int(x * 256), 255) into
 *                         map_table[i], 256 x 3 DEVICE doubles.
 *                         flow panels (0..12): fp32 [H,W,2] and its maxrad -> [H,W,3], the Middlebury colour code of flow_to_image
 *                         in double from the divisor maxrad + 2^-52 on; flow_u8: the uint8 image, else fp32(double(byte) / 255.0).
 * rank, weight and the pointer lists (image, magnitude, mag_out, flow, rgb_src, ...) are HOST arrays; what they point to is on the device.
 * Refused before a launch, DYN_E_INVALID: counts outside the limits, a null pointer in a list, H or W below 1, H*W*3 >= 2^31, a rank
 * outside 0..n-1, a weight outside 0..1 (n = 1 passes 1.0), pointers that are not aligned to their element. */
int dyn_viewlog_ranges(int K, int H, int W, const void* image, const int32_t* magnitude, const void* mag_out, const int32_t* rank,
                       const double* weight, double* ranges, void* stream);
int dyn_viewlog_flow_max(int F, int H, int W, const void* flow, float* maxrad, void* stream);
typedef struct {
  int H, W;
  int n_rgb;                   /* 0..8 */
  const void* rgb_src;         /* HOST list of n_rgb DEVICE pointers, fp32 [H,W,3] */
  const int32_t* rgb_clamp;    /* HOST [n_rgb] 0 / 1 */
  const void* rgb_dst;         /* HOST list of n_rgb DEVICE pointers, fp32 [3,H,W] */
  int n_map;                   /* 0..4 */
  const void* map_src;         /* HOST list of n_map DEVICE pointers, fp32 [H,W] */
  const void* map_table;       /* HOST list of n_map DEVICE pointers, double [256,3] */
  const double* ranges;        /* DEVICE [n_map][2] (dyn_viewlog_ranges) */
  const void* map_dst;         /* HOST list of n_map DEVICE pointers, double [3,H,W] or [H,W,3] */
  int map_chw;
  int n_flow;                  /* 0..12 */
  const void* flow_src;        /* HOST list of n_flow DEVICE pointers, fp32 [H,W,2] */
  const float* maxrad;         /* DEVICE [n_flow] (dyn_viewlog_flow_max) */
  const void* flow_dst;        /* HOST list of n_flow DEVICE pointers, fp32 or uint8 [H,W,3] */
  int flow_u8;
} DynViewLogPanelsParams;
int dyn_viewlog_panels(const DynViewLogPanelsParams* p, void* stream);

/* ====== the optimizer step of the training loop (train.py:199, :467 model.optimizer.step(); ibrnet/model.py:341-364 torch.optim.Adam) =========
 * ONE launch updates every tensor of every parameter group.  The grid is a list of chunks of DYN_ADAM_CHUNK elements: chunk c is elements
 * chunks[c][1] * DYN_ADAM_CHUNK ... of tensor chunks[c][0]; the list depends on the sizes alone and is uploaded once per parameter set.  The
 * per-tensor records change with every step (the gradient's address, the scalars that depend on the tensor's own step count and on the
 * group's learning rate) and are uploaded by the caller before the launch, on the same stream.
 * Per element, fp32, every operation rounded once (no fma), division and square root correctly rounded, subnormals kept:
 *     m = m + c1 * (g - m)          v = v * beta2 + (c2 * g) * g          denom = sqrtf(v) / s2 + eps          p = p + (a * m) / denom
 * with c1 = fp32(1 - beta1), c2 = fp32(1 - beta2), s2 = fp32(sqrt(1 - beta2^t)), a = fp32(-lr / (1 - beta1^t)), t the tensor's step count
 * after its increment, all formed by the host in double and rounded once.  A record with skip != 0 (a parameter without a gradient) is
 * left alone: p, g, m, v are not read.  With zero_grads the kernel stores 0 to g after reading it.  A chunk whose four pointers are all
 * 16-byte aligned at its first element moves float4s, any other chunk single floats; n < 2^31 per tensor.
 * Refused before a launch, DYN_E_INVALID: null params, records or chunks, counts below 1, records not on 8 bytes, chunks not on 8 bytes.
 * The kernel leaves a chunk alone whose tensor index or first element lies outside the records. */
#define DYN_ADAM_CHUNK 4096
typedef struct {
  float *p, *g, *m, *v;        /* DEVICE fp32 [n]: parameter, gradient, first and second moment, 4-byte aligned */
  int64_t n;                   /* elements, 1 .. 2^31 - 1 */
  float a, s2;                 /* depend on the step count and the learning rate */
  float c1, c2, beta2, eps;    /* depend on the group's options */
  int32_t skip;                /* 1: no gradient this step, the tensor is not touched */
  int32_t reserved;
} DynAdamTensor;
typedef struct {
  const void* tensors;         /* DEVICE [n_tensors] DynAdamTensor, 8-byte aligned */
  int n_tensors;
  const int32_t* chunks;       /* DEVICE [n_chunks][2]: tensor index, chunk index within the tensor; 8-byte aligned */
  int n_chunks;
  int zero_grads;              /* 0 / 1 */
} DynAdamParams;
int dyn_adam_step(const DynAdamParams* p, void* stream);

/* ------ the guard of the step: the global gradient norm, clipping by it, skipping a step whose gradients are not finite -----------------
 * Three plain launches in stream order over the records and the chunk list of dyn_adam_step: k_grad_sumsq (one workgroup per chunk) and
 * k_grad_stats (one workgroup) by dyn_grad_norm, then k_adam_step_guarded (or k_grad_scale for a stand-alone clip).  No atomics, no
 * counters between workgroups, nothing read back by the host.  The norm reads only g, n and skip of a record.  Every bit is decided here:
 *   chunk sum    One workgroup of 256 threads per chunk.  Element e of a chunk (0 <= e < len <= DYN_ADAM_CHUNK) belongs to lane
 *                (e >> 2) & 255 -- the float4 assignment of k_adam_step -- whatever the alignment of g: a chunk read in single floats sums
 *                the same elements per lane in the same order as one read in float4s.  A lane starts from 0.0 and adds
 *                (double)g[e] * (double)g[e] for its elements in increasing e; the product of two fp32 values is exact in double
 *                (subnormals included), each addition is rounded once.  The 256 lane sums are reduced within each wave of 64 by
 *                v += shfl_xor(v, m) for m = 32, 16, 8, 4, 2, 1, and the four wave sums are added as ((w0 + w1) + w2) + w3.  The result
 *                goes to partials[c]; a chunk whose record has skip != 0, or whose tensor index or first element lies outside the
 *                records, stores 0.0.  Every entry of partials is written by every call: it never needs clearing.
 *   finish       One workgroup of 256 threads.  Lane l adds partials[l], partials[l + 256], ... in that order from 0.0; the same
 *                reduction gives sumsq.  finite = isfinite(sumsq): the squares cannot overflow double, so finite is 0 exactly when some
 *                gradient element is Inf or NaN.  norm = (float)sqrt(sumsq), the correctly rounded double square root rounded to fp32
 *                once; norm can be +Inf while finite == 1 (two elements of 3e38: sumsq = 1.8e77).  coef in fp32, every operation rounded
 *                once: 1.0f when max_norm <= 0 or finite == 0, otherwise fminf(1.0f, max_norm / (norm + 1e-6f)) -- torch's
 *                clip_grad_norm_ with one correctly rounded division.  An infinite norm under clipping therefore gives coef = 0: the
 *                guarded step then moves the parameters by the moments alone.  With count != 0 one thread does calls += 1 and, when
 *                finite == 0, nonfinite += 1, by plain loads and stores (one workgroup; calls are ordered by the stream).
 *   guarded step The grid, the paths and the data movement of k_adam_step.  Every workgroup reads stats->coef and stats->finite.  If
 *                skip_nonfinite != 0 and finite == 0: p, m and v are not written; with zero_grads the gradients are still cleared.
 *                Otherwise g' = g * coef (one fp32 multiplication; coef == 1 is the identity), then the update of dyn_adam_step on g'.
 *                g itself is never rewritten with g': the step stores no gradients other than the zeros of zero_grads.
 *   scale        g = g * stats->coef in place for every record with skip == 0 (one fp32 multiplication per element); with coef == 1
 *                nothing is written.
 * Refused before a launch, DYN_E_INVALID: null params, records, chunks, partials or stats (each where the call takes it), counts below 1,
 * records, chunks, partials or stats not on 8 bytes, a NaN max_norm. */
typedef struct {
  double  sumsq;               /* sum of g*g over every element of every record with skip == 0 */
  float   norm;                /* (float)sqrt(sumsq): double sqrt, then one rounding to fp32 */
  float   coef;                /* the clip factor */
  int32_t finite;              /* 1 when sumsq is finite, i.e. when every gradient element is */
  int32_t reserved;
  int64_t calls;               /* += 1 per dyn_grad_norm call with count != 0 */
  int64_t nonfinite;           /* += 1 per such call with finite == 0 */
} DynGradStats;                /* DEVICE, 8-byte aligned; the caller zeroes it once */
typedef struct {
  const void* tensors;         /* DEVICE [n_tensors] DynAdamTensor, 8-byte aligned: g, n and skip are read */
  int n_tensors;
  const int32_t* chunks;       /* DEVICE [n_chunks][2], as for dyn_adam_step */
  int n_chunks;
  double* partials;            /* DEVICE [n_chunks], written in full */
  DynGradStats* stats;         /* DEVICE */
  float max_norm;              /* <= 0: no clipping (coef = 1) */
  int count;                   /* != 0: calls and nonfinite advance */
} DynGradNormParams;
int dyn_grad_norm(const DynGradNormParams* p, void* stream);
typedef struct {
  const void* tensors;
  int n_tensors;
  const int32_t* chunks;
  int n_chunks;
  const DynGradStats* stats;   /* DEVICE: coef is read */
} DynGradScaleParams;
int dyn_grad_scale(const DynGradScaleParams* p, void* stream);
typedef struct {
  const void* tensors;         /* the fields of DynAdamParams ... */
  int n_tensors;
  const int32_t* chunks;
  int n_chunks;
  int zero_grads;
  int skip_nonfinite;          /* 0 / 1 */
  const DynGradStats* stats;   /* DEVICE: coef and finite are read (dyn_grad_norm on the same stream before this call) */
} DynAdamGuardedParams;
int dyn_adam_step_guarded(const DynAdamGuardedParams* p, void* stream);

/* ------ the extended step: weight decay (coupled and decoupled), amsgrad, maximize, device-resident step counts -------------------------
 * dyn_adam_step and dyn_adam_step_guarded above are what they were; a caller none of whose tensors needs an option below keeps calling them.
 * The extended step has its own record, DynAdamXTensor, its own kernels (k_adamx_step, k_adamx_step_guarded: the grid, the chunk list, the
 * float4 / single-float choice -- vmax joins the alignment test when it is not null --, zero_grads and the guard's wave-uniform way out of
 * the kernels above) and one more kernel, k_adam_advance.  Per element, fp32, every operation rounded once (no fma), division and square
 * root correctly rounded, subnormals kept, in this order:
 *     g1 = (flags & 1) ? -g : g                                    maximize
 *     g2 = g1 * coef                                               the guarded form only (coef == 1 is the identity)
 *     g3 = (wd != 0) ? g2 + (wd * p) : g2                          coupled decay: two roundings; wd == 0 adds nothing (not even +0)
 *     p1 = p * decay                                               decoupled decay, decay = fp32(1 - lr * lambda) formed by the host in double;
 *                                                                  decay == 1 is the identity.  The moments see the undecayed gradient g3 and
 *                                                                  the coupled term reads the undecayed p, as in torch's AdamW / Adam.
 *     m = m + c1 * (g3 - m)          v = v * beta2 + (c2 * g3) * g3
 *     vmax != null:  vmax = (v > vmax) ? v : vmax,  d = vmax       amsgrad; otherwise d = v.  A NaN v leaves vmax as it is, where
 *                                                                  torch.maximum would store the NaN: the only difference from torch's
 *                                                                  amsgrad, and skip_nonfinite is what keeps NaN out of v in the first place.
 *     denom = sqrtf(d) / s2 + eps    p = p1 + (a * m) / denom
 * The guard's norm (dyn_grad_norm, over DynAdamTensor records of the same tensors) is taken over the raw gradients g, as clip_grad_norm_ in
 * front of a torch step would.
 * Device-resident step counts: a record with pow != null takes a and s2 from the device instead of the record.  pow[0], pow[1] hold
 * beta1^t, beta2^t of the t steps the tensor has taken (1.0, 1.0 before the first), step holds t as fp32.  Every workgroup of the tensor
 * forms, in double, every operation rounded once,
 *     b1 = pow[0] * beta1_d     b2 = pow[1] * beta2_d     a = (float)(-lr_d / (1.0 - b1))     s2 = (float)sqrt(1.0 - b2)
 * and only reads that state.  k_adam_advance (one thread per record, launched after the step in stream order when advance != 0) then
 * stores step + 1.0f, b1 and b2 for every record with pow != null and skip == 0 -- unless the step was held (skip_nonfinite != 0 and
 * finite == 0), which leaves p, m, v, vmax, step and pow bit for bit as they were.  No workgroup reads state another one has written in
 * the same launch; nothing is read back by the host.
 * Refused before a launch, DYN_E_INVALID: what dyn_adam_step / dyn_adam_step_guarded refuse. */
typedef struct {
  float *p, *g, *m, *v;        /* as DynAdamTensor */
  int64_t n;
  float a, s2;                 /* read when pow == null */
  float c1, c2, beta2, eps;
  int32_t skip;
  int32_t flags;               /* bit 0: maximize */
  float* vmax;                 /* DEVICE fp32 [n], null: no amsgrad */
  float wd;                    /* the coupled lambda, 0: none */
  float decay;                 /* the decoupled factor, 1: none */
  double* pow;                 /* DEVICE [2], 8-byte aligned, null: a and s2 above.  Read by the step, written by k_adam_advance alone */
  float* step;                 /* DEVICE fp32 scalar, required with pow.  Written by k_adam_advance alone */
  double lr_d, beta1_d, beta2_d; /* read with pow */
} DynAdamXTensor;
typedef struct {
  const void* tensors;         /* DEVICE [n_tensors] DynAdamXTensor, 8-byte aligned */
  int n_tensors;
  const int32_t* chunks;       /* as for dyn_adam_step */
  int n_chunks;
  int zero_grads;
  int advance;                 /* != 0: some record has pow != null, k_adam_advance follows the step */
} DynAdamXParams;
int dyn_adamx_step(const DynAdamXParams* p, void* stream);
typedef struct {
  const void* tensors;
  int n_tensors;
  const int32_t* chunks;
  int n_chunks;
  int zero_grads;
  int advance;
  int skip_nonfinite;
  const DynGradStats* stats;   /* DEVICE: coef and finite are read */
} DynAdamXGuardedParams;
int dyn_adamx_step_guarded(const DynAdamXGuardedParams* p, void* stream);

/* ====== scene preparation (save_monocular_cameras.py:90-113, monocular.py:125-204, eval_nvidia.py:387-428) ====================================
 * The resizes the reference takes from cv2, the erosion it takes from skimage and np.percentile of a depth map, on B images per launch.
 * The contracts restate OpenCV's and skimage's algorithms; whether they agree with the real libraries is BELIEVED, NOT VERIFIED.
 * src is contiguous, [B] images of the stated layout.  dst image b starts at dst + b * dst_pitch (BYTES) and is contiguous within itself; the
 * bytes between the end of an image and the next one (the padding of a pitched store) are never written.  Nothing is allocated.
 * For an axis of source size s and destination size d: scale = 1.0 / ((double)d / s).
 *   dyn_resize_area_u8     cv2.resize(INTER_AREA) shrinking uint8 [B,Hs,Ws,C], C in 1, 3, 4 -> [B,Hd,Wd,C].  Both scales integers
 *                          (|scale - (int)scale| < DBL_EPSILON): the integer sum of the ix * iy block; (sum + 2) >> 2 for 2 x 2, else
 *                          rintf((float)sum * (1.f / (ix * iy))), saturated; the tables are not read and may be null.  Otherwise the
 *                          decimation tables of both axes (DEVICE; built by the caller in double and rounded to fp32; destination index i
 *                          has count[i] <= K entries (idx[i][k], w[i][k])): for destination index i, f1 = i * scale, f2 = f1 + scale,
 *                          cell = min(scale, s - f1), s1 = ceil(f1), s2 = min(floor(f2), s - 1), s1 = min(s1, s2); entries in this order:
 *                          (s1 - 1, (s1 - f1) / cell) if s1 - f1 > 1e-3; (k, 1 / cell) for k in [s1, s2); (s2, min(min(f2 - s2, 1), cell)
 *                          / cell) if f2 - s2 > 1e-3.  fp32, one rounded operation at a time: per source row a destination pixel starts
 *                          at 0.f and adds (float)S[k] * alpha over the x entries in order; the destination row is the sequential sum
 *                          of beta * rowvalue over the y entries, the first term initialising it; rintf (ties to even), saturated.
 *                          Table indices are clamped to the source, counts to K.
 *   dyn_resize_area_f32    cv2.resize(INTER_AREA) on fp32 [B,Hs,Ws,C], C in 1..4 -> [B,Hd,Wd,C], shrinking AND enlarging; dst_pitch a multiple
 *                          of 4.  The branch is OpenCV's.  (1) Neither axis enlarges and both scales are integers (the test above): equal
 *                          sizes are a copy, bit for bit; else sum = 0.f over the ix * iy block in row-major order k = q * ix + p, in the
 *                          order of OpenCV's scalar loop: while four or more taps remain sum = sum + (((S[k] + S[k+1]) + S[k+2]) + S[k+3]),
 *                          then the rest one at a time; out = sum * (1.f / (ix * iy)).  (OpenCV's 2 x 2 SIMD path may associate
 *                          differently; the scalar order is the contract.)  (2) Neither axis enlarges, a scale is not an integer: the
 *                          decimation tables and the arithmetic of dyn_resize_area_u8 without the rintf and the saturation.  (3) An axis
 *                          enlarges (Hd > Hs or Wd > Ws): OpenCV's two-tap linear kernel with area-mode coefficients on BOTH axes, also the
 *                          one that shrinks; the tables are not read.  With inv = (double)d / s and scale = 1.0 / inv, destination index i
 *                          has s0 = floor(i * scale) in double and f = (float)((i + 1) - (s0 + 1) * inv) with the inner arithmetic in
 *                          double, then in fp32 f = f <= 0 ? 0 : f - floorf(f).  Edges and order as dyn_resize_linear_f32: horizontally
 *                          s0 >= Ws - 1 -> the value is S[Ws - 1], no second tap, else S[s0] * (1.f - f) + S[s0 + 1] * f; vertically rows
 *                          s0, s0 + 1 clamped to Hs - 1, r0 * (1.f - f) + r1 * f, weights not zeroed; horizontal first, every product and
 *                          sum rounded on its own.  Like the rest of this section a restatement of OpenCV from memory: BELIEVED, NOT VERIFIED.
 *   dyn_resize_linear_f32  cv2.resize(INTER_LINEAR) on fp32 [B,Hs,Ws] -> [B,Hd,Wd].  Per destination index i: f = (float)((i + 0.5) *
 *                          scale - 0.5) with the inner arithmetic in double, s0 = floor(f), f = f - (float)s0 in fp32.  Horizontally:
 *                          s0 < 0 -> s0 = 0, f = 0; s0 >= Ws - 1 -> the value is S[Ws - 1], no second tap; else S[s0] * (1.f - f) +
 *                          S[s0 + 1] * f.  Vertically rows s0, s0 + 1 clamped to [0, Hs - 1], weights (1.f - f) and f NOT zeroed at the
 *                          edges: r0 * (1.f - f) + r1 * f.  Horizontal first, every product and sum rounded on its own.  reciprocal: a
 *                          tap is 1.f / S (the disparity of a depth map); divide: the result is divided by divisor (non-zero) in fp32.
 *   dyn_resize_nearest     cv2.resize(INTER_NEAREST) on pixels of 1, 3, 4, 8 or 12 bytes: source index min((int)floor(i * scale), s - 1)
 *                          per axis, in double.  below >= 0: the destination is uint8 [B,Hd,Wd], (first byte of the pixel < below) ? 1 : 0
 *                          (below = 255 is the loader's 1 - m / 255 > 1e-3 on a decoded uint8 m); below = -1: the pixel is copied.
 *   dyn_erode_disk_u8      skimage.morphology.erosion(mask, disk(radius)) on 0 / 1 uint8 [B,H,W], radius 0..15: out = AND over the IN-IMAGE
 *                          (y + dy, x + dx) with dx*dx + dy*dy <= radius*radius of (src != 0); src and dst must not overlap.
 *   dyn_percentile_pair    two percentiles by numpy's `linear` method for each of B fp32 images of n values, image b at x + b * stride
 *                          (elements).  rank[4] (HOST): the order statistics below and above each percentile; weight[2] (HOST): the
 *                          interpolation weights; as dyn_viewlog_ranges selects them.  single: fp32 arithmetic throughout, out fp32
 *                          [B][2] (np.percentile(x, q) with a scalar q); else a + fp32(b - a) t in double, out double [B][2].  DEVICE out.
 * Refused before a launch, DYN_E_INVALID: null or misaligned pointers, sizes below 1, an image of 2^31 bytes or more, B or Hd above 65535,
 * a dst_pitch smaller than an image, an enlarging INTER_AREA, a missing table, C / pixel_bytes / radius / below / rank / weight outside
 * their ranges. */
int dyn_resize_area_u8(int B, int Hs, int Ws, int C, int Hd, int Wd, const void* src, void* dst, int64_t dst_pitch, const int32_t* xcount,
                       const int32_t* xidx, const float* xw, int Kx, const int32_t* ycount, const int32_t* yidx, const float* yw, int Ky,
                       void* stream);
int dyn_resize_area_f32(int B, int Hs, int Ws, int C, int Hd, int Wd, const float* src, float* dst, int64_t dst_pitch, const int32_t* xcount,
                        const int32_t* xidx, const float* xw, int Kx, const int32_t* ycount, const int32_t* yidx, const float* yw, int Ky,
                        void* stream);
int dyn_resize_linear_f32(int B, int Hs, int Ws, int Hd, int Wd, const float* src, float* dst, int64_t dst_pitch, int reciprocal, int divide,
                          float divisor, void* stream);
int dyn_resize_nearest(int B, int Hs, int Ws, int pixel_bytes, int Hd, int Wd, const void* src, void* dst, int64_t dst_pitch, int below,
                       void* stream);
int dyn_erode_disk_u8(int B, int H, int W, int radius, const void* src, void* dst, int64_t dst_pitch, void* stream);
int dyn_percentile_pair(int B, int64_t n, const float* x, int64_t stride, const int32_t* rank, const double* weight, int single, void* out,
                        void* stream);

/* ====== flow supervision (flow_utils.py:6-15 and the forward-backward check built on it) =====================================================
 * From raw optical flow to what a DeviceScene takes as flow_masks, plus the epipolar error of every flow vector under the scene's cameras.
 * Plain DEVICE pointers, contiguous arrays, nothing is allocated.  The contract is IEEE operations in a stated order: every product and sum
 * below is rounded on its own (no fused multiply-add), so a numpy restatement reproduces every output bit.  That the subpixel = 32 branch
 * agrees with cv2.remap (1/32-pixel fixed-point coordinates, the per-tap constant border, rint) is BELIEVED, NOT VERIFIED: cv2 was not
 * available.  alpha1 and alpha2 are parameters; nothing is claimed about the values any upstream preprocessing script uses.
 *   dyn_flow_resize       raw flow fp32 [B,Hs,Ws,2] -> [B,Hd,Wd,2]: each channel by the contract of dyn_resize_linear_f32 (no reciprocal, no
 *                         divisor), then u * (float)((double)Wd / Ws) and v * (float)((double)Hd / Hs), one rounded product each: numpy's
 *                         flow *= ratio on a float32 array.  Hs == Hd and Ws == Wd: a copy, bit for bit.
 *   dyn_warp_flow         flow_utils.warp_flow: img fp32 [B,H,W,C], 1 <= C <= 4, flow [B,H,W,2] -> out [B,H,W,C].  In fp32, per pixel
 *                         (row, col) with flow (u, v): mx = (float)col + u, my = (float)row + v; mx is clamped to [-2, (float)(W + 1)], my to
 *                         [-2, (float)(H + 1)], NaN becomes -2 (no result with a tap inside the image changes).  subpixel = 32: s = rint(mx *
 *                         32) (ties to even), ix = s >> 5 (floor), ax = (float)(s & 31) / 32; subpixel = 0: ix = floor(mx), ax = mx - floor(mx);
 *                         the same in y.  Weights w00 = (1-ax)*(1-ay), w01 = ax*(1-ay), w10 = (1-ax)*ay, w11 = ax*ay; taps t00 = img[iy][ix],
 *                         t01 = img[iy][ix+1], t10 = img[iy+1][ix], t11 = img[iy+1][ix+1], a tap outside the image is 0 and is not read
 *                         (BORDER_CONSTANT, per tap); out = ((t00*w00 + t01*w01) + t10*w10) + t11*w11.
 *   dyn_flow_supervision  one launch over a scene.  flows fp32 [N,6,H,W,2] in the order of the offsets +1, +2, +3, -1, -2, -3.  The partner of
 *                         frame i, slot j with offset o is frame i + o, slot (j + 3) % 6; the pair is in range iff 0 <= i + o < N.  An
 *                         out-of-range pair writes mask 0 and epi 0 and casts no vote.  Else, with f the own flow and w the partner's flow
 *                         plane warped by f (dyn_warp_flow, C = 2), in double from the fp32 values: a = f.u + w.u, b = f.v + w.v,
 *                         e = sqrt(a*a + b*b), t = alpha1 * (sqrt(f.u*f.u + f.v*f.v) + sqrt(w.u*w.u + w.v*w.v)) + alpha2, mask = e < t
 *                         (false for NaN: non-finite flow gives 0).  masks uint8 [N,6,H,W].
 *                         F double [N,6,9] or null: row-major fundamental matrices, x2^T F x1 = 0 for pixel x1 of frame i and its match x2
 *                         in frame i + o.  epi fp32 [N,6,H,W] or null, the Sampson distance in double: x = col, y = row, x2 = x + (double)u,
 *                         y2 = y + (double)v, l_k = (F[k][0]*x + F[k][1]*y) + F[k][2], m0 = (F[0][0]*x2 + F[1][0]*y2) + F[2][0],
 *                         m1 = (F[0][1]*x2 + F[1][1]*y2) + F[2][1], r = (x2*l0 + y2*l1) + l2, den = ((l0*l0 + l1*l1) + m0*m0) + m1*m1,
 *                         epi = den > 0 ? (float)(|r| / sqrt(den)) : 0; a non-finite own flow gives 0.  motion uint8 [N,H,W] or null:
 *                         (the number of in-range j with mask_j == 1 and epi_j > epi_thresh) >= min_votes, on the fp32 epi as stored.
 *                         epi and motion need F.
 * Refused before a launch, DYN_E_INVALID: N or B below 1, H or W below 1, H * W >= 2^31, C outside 1..4, a subpixel other than 0 or 32, null
 * or misaligned pointers (flows and F on 8 bytes, the rest on 4), an output that is an input, epi or motion without F, a NaN parameter. */
int dyn_flow_resize(int B, int Hs, int Ws, int Hd, int Wd, const float* src, float* dst, void* stream);
int dyn_warp_flow(int B, int H, int W, int C, const float* img, const float* flow, float* out, int subpixel, void* stream);
int dyn_flow_supervision(int N, int H, int W, const float* flows, const double* F, double alpha1, double alpha2, int subpixel, float epi_thresh,
                         int min_votes, void* masks, float* epi, void* motion, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DYNIBAR_HIP_H_ */
