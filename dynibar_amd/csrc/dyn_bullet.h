// The output stage of a rendered frame (render_monocular_bt.py:342-361 without the host work): up to four fp32 images [H,W,3] become one
// uint8 block [K, H - 2 crop_h, (W - 2 crop_w) * (2 with a ground-truth frame, else 1), 3], clipped, scaled, truncated and cropped on the
// device, so that one small device-to-host copy replaces three fp32 images and numpy.  (The input side of such a frame is k_scene_views with
// a target camera, dyn_scene.h, and the existing k_image_rays.)
// Included from dyn_geometry.hip: -ffp-contract=off; 255.0f * x below is one fp32 multiply like numpy's `255 * x` on a float32 array.
//
//   k_frame_pack_u8   one thread per output dword: four consecutive output bytes, so a wavefront stores 256 contiguous bytes.  The first
//                     byte's (image, row, byte within the output row) comes from two divisions, the next three by stepping; each byte maps
//                     back to a float of the cropped source row (consecutive bytes read consecutive floats) or, in the left half of a row
//                     with a ground truth, to a byte of the stored frame.  The last n mod 4 bytes are a scalar tail of one thread.
//                     The kernel is launch-bound at video sizes (about 1.6 MB in, 0.4 MB out at 288 x 512): DESIGN.md section 4.11.
#pragma once

#define FPK_THREADS 256

// (255 * np.clip(x, 0, 1)).astype(np.uint8) for every x but NaN, which is 0 here (numpy's cast of NaN depends on the platform).
// -inf, negatives and -0.0 give 0, +inf and x > 1 give 255.
__device__ __forceinline__ unsigned fpk_byte(float x) {
  if (!(x > 0.f)) return 0u;  // NaN too
  if (x >= 1.f) return 255u;
  return (unsigned)(255.0f * x);
}

struct FpkCursor {
  int k, row;
  long c;  // byte within the output row
};

__device__ __forceinline__ unsigned fpk_at(const DynFramePackParams& p, const uint8_t* __restrict__ gt, const FpkCursor& q, long wpred) {
  const long src0 = ((long)(q.row + p.crop_h) * p.W + p.crop_w) * 3;  // the first value of the cropped source row
  long c = q.c;
  if (p.gt_frame >= 0) {  // (gt null: a ground truth that the host check would have refused -- zeros in its half, nothing read)
    if (c < wpred) return gt ? gt[src0 + c] : 0u;
    c -= wpred;
  }
  const float* __restrict__ img = q.k == 0 ? p.image0 : q.k == 1 ? p.image1 : q.k == 2 ? p.image2 : p.image3;
  return fpk_byte(img[src0 + c]);
}

__global__ __launch_bounds__(FPK_THREADS) void k_frame_pack_u8(DynFramePackParams p) {
  const int hc = p.H - 2 * p.crop_h, wc = p.W - 2 * p.crop_w;
  if (hc < 1 || wc < 1 || p.crop_h < 0 || p.crop_w < 0 || p.K < 1 || p.K > 4) return;  // (refused before the launch)
  const bool gt_ok = p.frames && p.gt_frame >= 0 && p.gt_frame < p.N;
  const uint8_t* __restrict__ gt = gt_ok ? p.frames + (long)p.gt_frame * p.image_stride : nullptr;
  const long wpred = (long)wc * 3;                           // bytes of a predicted row
  const long wrow = (p.gt_frame >= 0 ? 2 : 1) * wpred;       // bytes of an output row
  const long n = (long)p.K * hc * wrow, ndw = n >> 2;
  const long j = (long)blockIdx.x * FPK_THREADS + threadIdx.x;
  if (j > ndw) return;
  const long e0 = 4 * j;
  FpkCursor q;
  q.k = (int)(e0 / (hc * wrow));
  const long rem = e0 - (long)q.k * (hc * wrow);
  q.row = (int)(rem / wrow);
  q.c = rem - (long)q.row * wrow;
  const int count = j < ndw ? 4 : (int)(n - e0);  // the tail thread: n mod 4 bytes
  unsigned w = 0u;
  for (int b = 0; b < count; ++b) {
    const unsigned v = fpk_at(p, gt, q, wpred);
    if (j < ndw) w |= v << (8 * b);
    else p.out[e0 + b] = (uint8_t)v;
    if (++q.c == wrow) {
      q.c = 0;
      if (++q.row == hc) { q.row = 0; ++q.k; }
    }
  }
  if (j < ndw) reinterpret_cast<unsigned*>(p.out)[j] = w;
}

extern "C" int dyn_frame_pack_u8(const DynFramePackParams* p, void* stream) {
  const char* who = "dyn_frame_pack_u8";
  DYN_REQUIRE(p, "%s: null params", who);
  DYN_REQUIRE(p->K >= 1 && p->K <= 4, "%s: K=%d images (1..4)", who, p->K);
  DYN_REQUIRE(p->H >= 1 && p->W >= 1 && (long)p->H * p->W * 3 < (1L << 31), "%s: H=%d W=%d is unsupported (H*W*3 < 2^31)", who, p->H, p->W);
  DYN_REQUIRE(p->crop_h >= 0 && p->crop_w >= 0 && p->H - 2L * p->crop_h >= 1 && p->W - 2L * p->crop_w >= 1,
              "%s: crops of %d rows and %d columns leave no pixel of %d x %d", who, p->crop_h, p->crop_w, p->H, p->W);
  const float* imgs[4] = {p->image0, p->image1, p->image2, p->image3};
  for (int k = 0; k < p->K; ++k) DYN_REQUIRE(imgs[k], "%s: image %d is null", who, k);
  DYN_REQUIRE(p->out, "%s: out is null", who);
  DYN_REQUIRE(((uintptr_t)p->out & 3) == 0, "%s: out must start on 4 bytes", who);
  if (p->gt_frame >= 0) {
    DYN_REQUIRE(p->frames, "%s: a ground-truth frame needs the store's frames", who);
    DYN_REQUIRE(p->gt_frame < p->N, "%s: ground-truth frame %d is outside 0..%d", who, p->gt_frame, p->N - 1);
    DYN_REQUIRE(p->image_stride >= (long)p->H * p->W * 3, "%s: image_stride=%ld is less than H*W*3", who, p->image_stride);
  } else {
    DYN_REQUIRE(p->gt_frame == -1, "%s: gt_frame=%d (-1: none)", who, p->gt_frame);
  }
  const long n = (long)p->K * (p->H - 2 * p->crop_h) * (p->W - 2 * p->crop_w) * 3 * (p->gt_frame >= 0 ? 2 : 1);
  DYN_LAUNCH(DYN_K_FRAME_PACK, who, k_frame_pack_u8, dim3(dyn_cdiv((n >> 2) + 1, FPK_THREADS)), dim3(FPK_THREADS), 0, (hipStream_t)stream, *p);
  return 0;
}
