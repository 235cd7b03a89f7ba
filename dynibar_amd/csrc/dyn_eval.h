// The inputs of a time step of the multi-camera benchmark evaluation (eval_nvidia.py:121-198 the item's image lists, :350-354 the masked
// static views, :423-444 the dynamic / static mask pair) from the device-resident scene of dyn_scene.h, without the host work.
// Included from dyn_geometry.hip: -ffp-contract=off; float(u8) / 255.0f is numpy's `astype(float32) / 255.0` and rgb * mask below is one
// fp32 multiply, torch's `static_src_rgbs * static_src_masks[:, None]`, bit for bit.
//
//   k_scene_views_masked  grid (tiles, V_src + V_static), one launch per TIME STEP (the lists do not depend on the target camera).  A
//                         workgroup takes a tile of 1024 pixels of its view: 768 image dwords and 256 mask dwords.  The image is read with
//                         k_scene_views' pattern -- lane l takes dword j + l, 256 bytes per wavefront and load, three loads per thread --
//                         and every dword becomes one float4 store (four scalar stores where view v of that output does not start on 16
//                         bytes).  A temporal view (v < V_src) is u8 / 255 alone.  A static view writes three outputs from that one read:
//                         the image, the mask as fp32 [H,W] and, when asked for, image * mask.  The product takes the mask of its two pixels
//                         per byte like k_scene_views does (the tile's own 1 KiB of mask, cached); the fp32 mask itself is the tile's mask
//                         dword tid, one float4 store per thread -- the same bytes of the same workgroup, so a mask is fetched from memory
//                         once.  A mask frame of -1 is the script's np.ones_like: exactly 1.0f, and the product image * 1.0f.
//                         The last H*W*3 mod 4 values of an image and H*W mod 4 of a mask are scalar tails of one thread each.  Workgroup 0
//                         of a view writes its camera.  Every index is checked again here and a bad view is written as zeros.
//   k_eval_mask_pair      a stored 0 / 1 mask of n = H*W*C bytes -> fp32 [2, n] = (m, 1.0f - m), m = float(byte): one dword read and two
//                         float4 stores per thread (the second half starts on 16 bytes when n is a multiple of 4, else scalar stores), a
//                         scalar tail of n mod 4 bytes.
#pragma once

#define EVS_THREADS 256
#define EVS_IMG_DWORDS 3  // image dwords per thread: a workgroup covers 768 dwords = 1024 pixels = 256 mask dwords

__device__ __forceinline__ void evs_store4(float* out, long j, bool vec, const float* f) {
  if (vec) {
    reinterpret_cast<float4*>(out)[j] = make_float4(f[0], f[1], f[2], f[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * j + c] = f[c];
  }
}

__device__ __forceinline__ bool evs_aligned(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One view of the step.  STATIC: the view also writes its fp32 mask (mout) and, where outm is not null, the masked image.
template <bool STATIC>
__device__ __forceinline__ void evs_view(const DynSceneStore& s, const int32_t* __restrict__ d, float* out, float* cam, float* mout, float* outm) {
  const int tid = threadIdx.x;
  const int frame = d[0], virt = d[1], mframe = d[2], kframe = d[3];
  const bool ok = frame >= 0 && frame < s.N && virt == -1 && mframe >= -1 && mframe < s.N && (STATIC || mframe == -1) &&
                  (mframe < 0 || (s.src_masks && s.mask_channels == 1)) && kframe >= 0 && kframe < s.N;
  const long HW = (long)s.H * s.W;
  const long n = HW * 3, ndw = n >> 2, mdw = HW >> 2;
  if (blockIdx.x == 0 && tid < 34) {
    float x = 0.f;  // [H, W, K(16), c2w(16)]: scn_camera for a stored frame that is no virtual view
    if (ok) x = tid == 0 ? (float)s.H : tid == 1 ? (float)s.W : tid < 18 ? s.intrinsics[(long)kframe * 16 + (tid - 2)] : s.poses[(long)frame * 16 + (tid - 18)];
    cam[tid] = x;
  }
  const bool vec = evs_aligned(out);
  const uint8_t* img = ok ? s.frames + (long)frame * s.image_stride : nullptr;
  const uint8_t* msk = (STATIC && ok && mframe >= 0) ? s.src_masks + (long)mframe * s.mask_stride : nullptr;
  const float fill = ok ? 1.0f : 0.f;  // the mask of a view without one; zeros for a view that was refused

  const long j0 = (long)blockIdx.x * (EVS_THREADS * EVS_IMG_DWORDS) + tid;
#pragma unroll
  for (int k = 0; k < EVS_IMG_DWORDS; ++k) {
    const long j = j0 + k * EVS_THREADS;
    if (j < ndw) {
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      if (img) {
        const unsigned w = reinterpret_cast<const unsigned*>(img)[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = scn_unit((w >> (8 * c)) & 255u);
      }
      evs_store4(out, j, vec, f);
      if (STATIC && outm) {
        const long p0 = (4 * j) / 3;  // the pixel of value 4j; the dword's four values lie in pixels p0 and p0 + 1
        float m0 = fill, m1 = fill;
        if (msk) {
          m0 = scn_unit(msk[p0]);
          m1 = scn_unit(msk[(4 * j + 3) / 3]);
        }
        float g[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) g[c] = f[c] * (((4 * j + c) / 3 == p0) ? m0 : m1);
        evs_store4(outm, j, evs_aligned(outm), g);
      }
    } else if (j == ndw) {  // the scalar tail of the image: n mod 4 values, one thread of the view
      for (long e = 4 * ndw; e < n; ++e) {
        const float x = img ? scn_unit(img[e]) : 0.f;
        out[e] = x;
        if (STATIC && outm) {
          float m = fill;
          if (msk) m = scn_unit(msk[e / 3]);
          outm[e] = x * m;
        }
      }
    }
  }
  if (STATIC) {
    const long i = (long)blockIdx.x * EVS_THREADS + tid;  // mask dword: the four pixels 4i .. 4i + 3 of this workgroup's tile
    if (i < mdw) {
      float f[4] = {fill, fill, fill, fill};
      if (msk) {
        const unsigned w = reinterpret_cast<const unsigned*>(msk)[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) f[c] = scn_unit((w >> (8 * c)) & 255u);
      }
      evs_store4(mout, i, evs_aligned(mout), f);
    } else if (i == mdw) {  // the scalar tail of the mask: H*W mod 4 values
      for (long e = 4 * mdw; e < HW; ++e) {
        float m = fill;
        if (msk) m = scn_unit(msk[e]);
        mout[e] = m;
      }
    }
  }
}

__global__ __launch_bounds__(EVS_THREADS) void k_scene_views_masked(DynSceneStore s, const int32_t* __restrict__ desc, int V_src, int V_static,
                                                                    float* src_rgbs, float* src_cameras, float* static_rgbs, float* static_masks,
                                                                    float* static_masked, float* static_cameras) {
  const int v = blockIdx.y;
  if (v >= V_src + V_static) return;
  const long HW = (long)s.H * s.W;
  if (v < V_src) {
    evs_view<false>(s, desc + v * 4, src_rgbs + (long)v * HW * 3, src_cameras + v * 34, nullptr, nullptr);
  } else {
    const int u = v - V_src;  // the view within the static list
    evs_view<true>(s, desc + v * 4, static_rgbs + (long)u * HW * 3, static_cameras + u * 34, static_masks + (long)u * HW,
                   static_masked ? static_masked + (long)u * HW * 3 : nullptr);
  }
}

__global__ __launch_bounds__(EVS_THREADS) void k_eval_mask_pair(const uint8_t* __restrict__ mask, long n, float* out) {
  const long ndw = n >> 2;
  const long j = (long)blockIdx.x * EVS_THREADS + threadIdx.x;
  float* inv = out + n;
  if (j < ndw) {
    const unsigned w = reinterpret_cast<const unsigned*>(mask)[j];
    float m[4], r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m[c] = (float)((w >> (8 * c)) & 255u);
      r[c] = 1.0f - m[c];
    }
    evs_store4(out, j, true, m);
    evs_store4(inv, j, (n & 3) == 0, r);
  } else if (j == ndw) {
    for (long e = 4 * ndw; e < n; ++e) {
      const float m = (float)mask[e];
      out[e] = m;
      inv[e] = 1.0f - m;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int dyn_scene_views_masked(const DynSceneStore* s, const int32_t* desc_host, const int32_t* desc, int V_src, int V_static,
                                      int want_masked, float* src_rgbs, float* src_cameras, float* static_rgbs, float* static_cameras,
                                      float* static_masks, float* static_masked, void* stream) {
  const char* who = "dyn_scene_views_masked";
  if (int rc = scn_check_store(s, who)) return rc;
  DYN_REQUIRE(V_src >= 1 && V_src <= SCN_MAX_VIEWS, "%s: %d temporal views (1..%d)", who, V_src, SCN_MAX_VIEWS);
  DYN_REQUIRE(V_static >= 1 && V_static <= SCN_MAX_VIEWS, "%s: %d static views (1..%d)", who, V_static, SCN_MAX_VIEWS);
  DYN_REQUIRE(desc_host && desc, "%s: desc_host and desc are required", who);
  DYN_REQUIRE(src_rgbs && src_cameras && static_rgbs && static_cameras && static_masks,
              "%s: src_rgbs, src_cameras, static_rgbs, static_cameras and static_masks are required", who);
  DYN_REQUIRE(want_masked == 0 || want_masked == 1, "%s: want_masked=%d (0 or 1)", who, want_masked);
  DYN_REQUIRE(!want_masked || static_masked, "%s: the masked static views were asked for but static_masked is null", who);
  DYN_REQUIRE(want_masked || !static_masked, "%s: static_masked was given but the masked static views were not asked for", who);
  DYN_REQUIRE(!s->src_masks || s->mask_channels == 1, "%s: the mask store has %d channels; a coarse mask is [H,W], one channel", who,
              s->mask_channels);
  const int V = V_src + V_static;
  for (int v = 0; v < V; ++v) {
    const int32_t* d = desc_host + v * 4;
    DYN_REQUIRE(d[0] >= 0 && d[0] < s->N, "%s: view %d: image frame %d is outside 0..%d", who, v, d[0], s->N - 1);
    DYN_REQUIRE(d[1] == -1, "%s: view %d: virtual index %d (an evaluation step has no virtual views: -1)", who, v, d[1]);
    DYN_REQUIRE(d[2] >= -1 && d[2] < s->N, "%s: view %d: mask frame %d is outside -1..%d", who, v, d[2], s->N - 1);
    DYN_REQUIRE(d[2] < 0 || v >= V_src, "%s: view %d is a temporal view and takes no mask, got mask frame %d", who, v, d[2]);
    DYN_REQUIRE(d[2] < 0 || s->src_masks, "%s: view %d asks for a coarse mask but the store has none", who, v);
    DYN_REQUIRE(d[3] >= 0 && d[3] < s->N, "%s: view %d: intrinsics frame %d is outside 0..%d", who, v, d[3], s->N - 1);
  }
  const long HW = (long)s->H * s->W;
  const int tiles = dyn_cdiv(((HW * 3) >> 2) + 1, EVS_THREADS * EVS_IMG_DWORDS);
  const int mtiles = dyn_cdiv((HW >> 2) + 1, EVS_THREADS);
  DYN_LAUNCH(DYN_K_SCENE_VIEWS_MASKED, who, k_scene_views_masked, dim3(tiles > mtiles ? tiles : mtiles, V), dim3(EVS_THREADS), 0,
             (hipStream_t)stream, *s, desc, V_src, V_static, src_rgbs, src_cameras, static_rgbs, static_masks,
             want_masked ? static_masked : nullptr, static_cameras);
  return 0;
}

extern "C" int dyn_eval_mask_pair(const uint8_t* mask, int H, int W, int C, float* out, void* stream) {
  const char* who = "dyn_eval_mask_pair";
  DYN_REQUIRE(H >= 1 && W >= 1 && (long)H * W * 3 < (1L << 31), "%s: H=%d W=%d is unsupported (H*W*3 < 2^31)", who, H, W);
  DYN_REQUIRE(C == 1 || C == 3, "%s: C=%d channels (1 or 3)", who, C);
  DYN_REQUIRE(mask, "%s: mask is null", who);
  DYN_REQUIRE(out, "%s: out is null", who);
  DYN_REQUIRE(((uintptr_t)mask & 3) == 0, "%s: mask must start on 4 bytes", who);
  DYN_REQUIRE(((uintptr_t)out & 15) == 0, "%s: out must start on 16 bytes", who);
  const long n = (long)H * W * C;
  DYN_LAUNCH(DYN_K_EVAL_MASK_PAIR, who, k_eval_mask_pair, dim3(dyn_cdiv((n >> 2) + 1, EVS_THREADS)), dim3(EVS_THREADS), 0, (hipStream_t)stream,
             mask, n, out);
  return 0;
}
