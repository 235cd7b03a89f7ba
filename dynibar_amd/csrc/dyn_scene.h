// Training batches from a device-resident scene (monocular.py:120-144, :300-425 and sample_ray.py:262-331 without the host work): the scene's
// frames, virtual views and source masks stay on the device as uint8, its disparities, masks and flows as they are, and one batch is two
// launches driven by a few dozen integers.
// Included from dyn_geometry.hip: the unit is built with -ffp-contract=off, and float(u8) / 255.0f below is a correctly rounded fp32
// division -- numpy's `astype(float32) / 255.0` bit for bit (dyn_metrics.h prepares its uint8 target by the same rule).
//
//   k_scene_views        grid (chunks, V).  View v of the batch is described by four integers (image frame, virtual index or -1, mask frame
//                        or -1, intrinsics frame).  Its H*W*3 bytes are read as dwords: within a wavefront lane l takes dword j + l of the
//                        image -- one fully coalesced 256-byte load -- and turns it into the four floats 4j .. 4j + 3 of the output, one
//                        float4 store per lane, 1 KiB per wavefront and instruction.  Per lane and pass of SCN_UNROLL dwords that is the
//                        work on four pixels (12 bytes in, three float4 out).  The store pads every image to a multiple of 16 bytes, so
//                        the dword loads are aligned whatever H*W*3 is; the float4 stores are used where view v of the OUTPUT starts on
//                        16 bytes (always when H*W*3 is a multiple of 4), four scalar stores otherwise.  The last H*W*3 mod 4 values are
//                        a scalar tail.  A one-channel mask is read per byte (two pixels at most per dword, cached), a three-channel mask
//                        as the image's own dword.  Workgroup 0 of a view writes its camera [H, W, K(16), c2w(16)].  With a target
//                        camera (dyn_scene_views_target: a frame rendered from a camera that is not one of the scene's, dyn_bullet.h) a
//                        view whose intrinsics frame is -1 takes K from that camera; without one -1 is a bad index like any other.
//   k_scene_supervision  one thread per selected pixel: ray (dyn_ray_basis / dyn_ray_dir, the code of k_image_rays: the same bits), pixel
//                        coordinates, rgb / 255, and copies of disparity, the two masks, the six flows and their masks.  Thread-sized
//                        gathers of a random pixel set (its measured time: DESIGN.md section 4.10).  Workgroup 0 also writes the two cameras.
//
// Both kernels check every index they were given against the store again and write zeros for a bad one: whatever the host passes, nothing is
// read out of bounds.  (The entry points refuse such a call before it is launched; the check in the kernel costs a comparison.)
#pragma once

#define SCN_THREADS 256
#define SCN_UNROLL 4      // dwords per thread of k_scene_views: a workgroup covers 1024 dwords = 1365 1/3 pixels
#define SCN_MAX_VIEWS 32  // per list: the network engine's own limit
#define SCN_FLOWS 6

__device__ __forceinline__ float scn_unit(unsigned b) { return (float)b / 255.0f; }

// intr_frame -1 (dyn_scene_views_target only): K of the target camera, a [34] array laid out like cam itself
__device__ __forceinline__ void scn_camera(const DynSceneStore& s, int pose_frame, int virt, int intr_frame, float* __restrict__ cam, int t,
                                           const float* __restrict__ target_camera = nullptr) {
  if (t == 0) cam[0] = (float)s.H;
  else if (t == 1) cam[1] = (float)s.W;
  else if (t < 18) cam[t] = intr_frame < 0 ? target_camera[t] : s.intrinsics[(long)intr_frame * 16 + (t - 2)];
  else if (t < 34) cam[t] = virt >= 0 ? s.vposes[((long)pose_frame * 8 + virt) * 16 + (t - 18)] : s.poses[(long)pose_frame * 16 + (t - 18)];
}

__global__ __launch_bounds__(SCN_THREADS) void k_scene_views(DynSceneStore s, const int32_t* __restrict__ desc, float* __restrict__ images,
                                                             float* __restrict__ cameras, const float* __restrict__ target_camera) {
  const int v = blockIdx.y, tid = threadIdx.x;
  const int frame = desc[v * 4], virt = desc[v * 4 + 1], mframe = desc[v * 4 + 2], kframe = desc[v * 4 + 3];
  const bool ok = frame >= 0 && frame < s.N && virt >= -1 && virt < 8 && (virt < 0 || (s.vviews && s.vposes)) && mframe >= -1 && mframe < s.N &&
                  (mframe < 0 || s.src_masks) && kframe >= (target_camera ? -1 : 0) && kframe < s.N;
  const long n = (long)s.H * s.W * 3;  // values of one image
  const long ndw = n >> 2;
  float* __restrict__ out = images + (long)v * n;
  const bool vec = ((((long)v * n) & 3) == 0) && ((reinterpret_cast<uintptr_t>(images) & 15) == 0);
  if (blockIdx.x == 0 && tid < 34) {
    if (ok) scn_camera(s, frame, virt, kframe, cameras + v * 34, tid, target_camera);
    else cameras[v * 34 + tid] = 0.f;
  }
  const uint8_t* img = nullptr;
  const uint8_t* msk = nullptr;
  if (ok) {
    img = virt >= 0 ? s.vviews + ((long)frame * 8 + virt) * s.image_stride : s.frames + (long)frame * s.image_stride;
    if (mframe >= 0) msk = s.src_masks + (long)mframe * s.mask_stride;
  }
  const long j0 = (long)blockIdx.x * (SCN_THREADS * SCN_UNROLL) + tid;
#pragma unroll
  for (int k = 0; k < SCN_UNROLL; ++k) {
    const long j = j0 + k * SCN_THREADS;
    if (j < ndw) {
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      if (img) {
        const unsigned w = reinterpret_cast<const unsigned*>(img)[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = scn_unit((w >> (8 * c)) & 255u);
        if (msk) {
          if (s.mask_channels == 3) {
            const unsigned m = reinterpret_cast<const unsigned*>(msk)[j];
#pragma unroll
            for (int c = 0; c < 4; ++c) f[c] = f[c] * scn_unit((m >> (8 * c)) & 255u);
          } else {
            const long p0 = (4 * j) / 3;  // the pixel of value 4j; the dword's four values lie in pixels p0 and p0 + 1
            const float m0 = scn_unit(msk[p0]), m1 = scn_unit(msk[(4 * j + 3) / 3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) f[c] = f[c] * (((4 * j + c) / 3 == p0) ? m0 : m1);
          }
        }
      }
      if (vec) {
        reinterpret_cast<float4*>(out)[j] = make_float4(f[0], f[1], f[2], f[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) out[4 * j + c] = f[c];
      }
    } else if (j == ndw) {  // the scalar tail: n mod 4 values, one thread of the view
      for (long e = 4 * ndw; e < n; ++e) {
        float x = 0.f;
        if (img) {
          x = scn_unit(img[e]);
          if (msk) x = x * scn_unit(s.mask_channels == 3 ? msk[e] : msk[e / 3]);
        }
        out[e] = x;
      }
    }
  }
}

__global__ __launch_bounds__(SCN_THREADS) void k_scene_supervision(DynSceneStore s, DynSceneSupervisionParams p) {
  const int r = blockIdx.x * SCN_THREADS + threadIdx.x;
  const bool frame_ok = p.frame >= 0 && p.frame < s.N;
  if (blockIdx.x == 0 && threadIdx.x < 34) {
    const int t = threadIdx.x;
    if (p.camera) {
      if (frame_ok) scn_camera(s, p.frame, -1, p.frame, p.camera, t);
      else p.camera[t] = 0.f;
    }
    if (p.anchor_camera) {
      if (p.anchor_frame >= 0 && p.anchor_frame < s.N) scn_camera(s, p.anchor_frame, -1, p.anchor_frame, p.anchor_camera, t);
      else p.anchor_camera[t] = 0.f;
    }
  }
  if (r >= p.R) return;
  const long HW = (long)s.H * s.W;
  const long pix = p.sel ? (long)p.sel[r] : (long)r;
  const bool ok = frame_ok && pix >= 0 && pix < HW;
  const long R = p.R;
  if (!ok) {
    for (int a = 0; a < 3; ++a) { p.ray_o[r * 3L + a] = 0.f; p.ray_d[r * 3L + a] = 0.f; p.rgb[r * 3L + a] = 0.f; }
    p.uv[r * 2L] = 0.f; p.uv[r * 2L + 1] = 0.f;
    p.disp[r] = 0.f; p.motion_mask[r] = 0.f; p.static_mask[r] = 0.f;
    for (int f = 0; f < SCN_FLOWS; ++f) { p.flows[(f * R + r) * 2] = 0.f; p.flows[(f * R + r) * 2 + 1] = 0.f; p.masks[f * R + r] = 0.f; }
    return;
  }
  const int px = (int)(pix % s.W), py = (int)(pix / s.W);
  const float u = (float)px, vv = (float)py;
  DynRayBasis b;
  dyn_ray_basis(s.intrinsics + (long)p.frame * 16, s.poses + (long)p.frame * 16, b);
  float d[3];
  dyn_ray_dir(b, u, vv, d);
  const uint8_t* img = s.frames + (long)p.frame * s.image_stride + pix * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p.ray_o[r * 3L + a] = b.o[a];
    p.ray_d[r * 3L + a] = d[a];
    p.rgb[r * 3L + a] = scn_unit(img[a]);
  }
  p.uv[r * 2L] = u;
  p.uv[r * 2L + 1] = vv;
  const long at = (long)p.frame * HW + pix;
  p.disp[r] = s.disp[at];
  p.motion_mask[r] = (float)s.motion_mask[at];
  p.static_mask[r] = (float)s.static_mask[at];
#pragma unroll
  for (int f = 0; f < SCN_FLOWS; ++f) {
    const long fa = ((long)p.frame * SCN_FLOWS + f) * HW + pix;
    const float2 fl = reinterpret_cast<const float2*>(s.flows)[fa];
    reinterpret_cast<float2*>(p.flows)[f * R + r] = fl;
    p.masks[f * R + r] = (float)s.flow_masks[fa];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static int scn_check_store(const DynSceneStore* s, const char* who) {
  DYN_REQUIRE(s, "%s: null store", who);
  DYN_REQUIRE(s->N >= 1 && s->H >= 1 && s->W >= 1, "%s: N=%d H=%d W=%d", who, s->N, s->H, s->W);
  DYN_REQUIRE((long)s->H * s->W * 3 < (1L << 31), "%s: H=%d W=%d is too large (H*W*3 < 2^31)", who, s->H, s->W);
  DYN_REQUIRE(s->frames && s->intrinsics && s->poses, "%s: frames, intrinsics and poses are required", who);
  DYN_REQUIRE(s->image_stride >= (long)s->H * s->W * 3 && s->image_stride % 16 == 0 && ((uintptr_t)s->frames & 15) == 0 &&
                  ((uintptr_t)s->vviews & 15) == 0,
              "%s: images must start on 16 bytes, image_stride=%ld a multiple of 16 and at least H*W*3", who, s->image_stride);
  if (s->src_masks) {
    DYN_REQUIRE(s->mask_channels == 1 || s->mask_channels == 3, "%s: mask_channels=%d (1 or 3)", who, s->mask_channels);
    DYN_REQUIRE(s->mask_stride >= (long)s->H * s->W * s->mask_channels && s->mask_stride % 16 == 0 && ((uintptr_t)s->src_masks & 15) == 0,
                "%s: masks must start on 16 bytes, mask_stride=%ld a multiple of 16 and at least H*W*channels", who, s->mask_stride);
  }
  return 0;
}

// The argument check and the launch of both entry points.  tcam_host / tcam: the target camera (host copy, DEVICE array) or null, and
// with null an intrinsics frame of -1 is refused like any other index out of range.
static int scn_views_launch(const char* who, const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_ref, int V_anchor,
                            int V_static, const float* tcam_host, const float* tcam, float* images, float* cameras, void* stream) {
  if (int rc = scn_check_store(s, who)) return rc;
  DYN_REQUIRE(desc_host && desc && images && cameras, "%s: desc_host, desc, images and cameras are required", who);
  DYN_REQUIRE(V_ref >= 0 && V_anchor >= 0 && V_static >= 0 && V_ref + V_anchor + V_static >= 1, "%s: view counts %d, %d, %d", who, V_ref,
              V_anchor, V_static);
  DYN_REQUIRE(V_ref <= SCN_MAX_VIEWS && V_anchor <= SCN_MAX_VIEWS && V_static <= SCN_MAX_VIEWS,
              "%s: %d, %d, %d views in the lists (at most %d per list)", who, V_ref, V_anchor, V_static, SCN_MAX_VIEWS);
  const int V = V_ref + V_anchor + V_static;
  const int kmin = tcam ? -1 : 0;
  for (int v = 0; v < V; ++v) {
    const int32_t* d = desc_host + v * 4;
    DYN_REQUIRE(d[0] >= 0 && d[0] < s->N, "%s: view %d: image frame %d is outside 0..%d", who, v, d[0], s->N - 1);
    DYN_REQUIRE(d[1] >= -1 && d[1] < 8, "%s: view %d: virtual index %d is outside -1..7", who, v, d[1]);
    DYN_REQUIRE(d[1] < 0 || (s->vviews && s->vposes), "%s: view %d is a virtual view but the store has none", who, v);
    DYN_REQUIRE(d[2] >= -1 && d[2] < s->N, "%s: view %d: mask frame %d is outside -1..%d", who, v, d[2], s->N - 1);
    DYN_REQUIRE(d[2] < 0 || s->src_masks, "%s: view %d asks for a source mask but the store has none", who, v);
    DYN_REQUIRE(d[3] >= kmin && d[3] < s->N, "%s: view %d: intrinsics frame %d is outside %d..%d", who, v, d[3], kmin, s->N - 1);
  }
  const long ndw = ((long)s->H * s->W * 3) >> 2;
  DYN_LAUNCH(DYN_K_SCENE_VIEWS, who, k_scene_views, dim3(dyn_cdiv(ndw + 1, SCN_THREADS * SCN_UNROLL), V), dim3(SCN_THREADS), 0,
             (hipStream_t)stream, *s, desc, images, cameras, tcam);
  return 0;
}

extern "C" int dyn_scene_views(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_ref, int V_anchor, int V_static,
                               float* images, float* cameras, void* stream) {
  return scn_views_launch("dyn_scene_views", s, desc_host, desc, V_ref, V_anchor, V_static, nullptr, nullptr, images, cameras, stream);
}

extern "C" int dyn_scene_views_target(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_ref, int V_anchor, int V_static,
                                      const float* target_camera_host, const float* target_camera, float* images, float* cameras, void* stream) {
  const char* who = "dyn_scene_views_target";
  if (int rc = scn_check_store(s, who)) return rc;
  DYN_REQUIRE((target_camera_host != nullptr) == (target_camera != nullptr), "%s: target_camera and its host copy go together", who);
  if (target_camera_host) {
    DYN_REQUIRE(target_camera_host[0] == (float)s->H && target_camera_host[1] == (float)s->W,
                "%s: the target camera is %g x %g, the scene's images are not", who, (double)target_camera_host[0], (double)target_camera_host[1]);
    for (int i = 2; i < 34; ++i) DYN_REQUIRE(target_camera_host[i] - target_camera_host[i] == 0.f, "%s: target camera entry %d is not finite", who, i);
  } else if (desc_host) {  // the one refusal that is this entry point's own: name the missing camera, not a range
    const int V = V_ref + V_anchor + V_static;
    if (V_ref >= 0 && V_anchor >= 0 && V_static >= 0 && V_ref <= SCN_MAX_VIEWS && V_anchor <= SCN_MAX_VIEWS && V_static <= SCN_MAX_VIEWS)
      for (int v = 0; v < V; ++v)
        DYN_REQUIRE(desc_host[v * 4 + 3] != -1, "%s: view %d takes the target camera's intrinsics (-1) but no target camera was given", who, v);
  }
  return scn_views_launch(who, s, desc_host, desc, V_ref, V_anchor, V_static, target_camera_host, target_camera, images, cameras, stream);
}

extern "C" int dyn_scene_supervision(const DynSceneStore* s, const DynSceneSupervisionParams* p, void* stream) {
  if (int rc = scn_check_store(s, "dyn_scene_supervision")) return rc;
  DYN_REQUIRE(p, "dyn_scene_supervision: null params");
  DYN_REQUIRE(s->disp && s->motion_mask && s->static_mask && s->flows && s->flow_masks,
              "dyn_scene_supervision: the store needs disp, motion_mask, static_mask, flows and flow_masks");
  DYN_REQUIRE(((uintptr_t)s->flows & 7) == 0 && ((uintptr_t)p->flows & 7) == 0, "dyn_scene_supervision: flows must be 8-byte aligned");
  DYN_REQUIRE(p->frame >= 0 && p->frame < s->N, "dyn_scene_supervision: frame %d is outside 0..%d", p->frame, s->N - 1);
  DYN_REQUIRE(!p->anchor_camera || (p->anchor_frame >= 0 && p->anchor_frame < s->N), "dyn_scene_supervision: anchor frame %d is outside 0..%d",
              p->anchor_frame, s->N - 1);
  DYN_REQUIRE(p->R >= 1, "dyn_scene_supervision: R=%d (at least 1)", p->R);
  DYN_REQUIRE(p->ray_o && p->ray_d && p->uv && p->rgb && p->disp && p->motion_mask && p->static_mask && p->flows && p->masks,
              "dyn_scene_supervision: every per-pixel output is required");
  const long HW = (long)s->H * s->W;
  if (p->sel) {
    DYN_REQUIRE(p->sel_host, "dyn_scene_supervision: sel_host (the host copy of sel) is required with sel");
    for (int r = 0; r < p->R; ++r)
      DYN_REQUIRE(p->sel_host[r] >= 0 && p->sel_host[r] < HW, "dyn_scene_supervision: pixel index %d (entry %d) is outside 0..%ld", p->sel_host[r], r,
                  HW - 1);
  } else {
    DYN_REQUIRE(p->R == HW, "dyn_scene_supervision: without sel R must be H*W = %ld, got %d", HW, p->R);
  }
  DYN_LAUNCH(DYN_K_SCENE_SUPERVISION, "dyn_scene_supervision", k_scene_supervision, dim3(dyn_cdiv(p->R, SCN_THREADS)), dim3(SCN_THREADS), 0,
             (hipStream_t)stream, *s, *p);
  return 0;
}
