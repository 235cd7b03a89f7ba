// Flow supervision from raw optical flow (flow_utils.py:6-15 and the forward-backward check built on it) on the device: the resize of a raw
// flow field, warp_flow (cv2.remap, INTER_LINEAR, BORDER_CONSTANT) and, in one launch over a scene, the consistency masks, the epipolar
// (Sampson) error of every flow vector and the vote that makes the geometric half of a motion mask.  The contract is restated in
// include/dynibar_hip.h (flow supervision); that the fixed-point branch agrees with cv2.remap is believed, not verified (cv2 was not available).
// Included from dyn_geometry.hip: -ffp-contract=off, and every function below that does arithmetic says so again with the pragma: every product
// and sum is rounded on its own, in the stated order, so a numpy restatement reproduces every output bit.
//
//   k_flow_resize       grid (cdiv(Wd, 256), rows, images): a lane makes the two values of one destination pixel with the taps and the order of
//                       k_resize_linear_f32 on each channel of the interleaved source, then multiplies u and v by the fp32 ratios.
//   k_warp_flow         grid (cdiv(W, 64), row tiles, images), tiles of 4 rows x 64 pixels: a lane owns a pixel and walks its C channels.
//   k_flow_supervision  the same tiles over (W, H, frames): a wave owns 64 neighbouring pixels of a row, so its own six flow vectors are six
//                       coalesced 512 B reads and its mask / epi stores are 64 B / 256 B runs; the four taps of a partner flow land within a few
//                       pixels of the lane's own position for flows of video size and are served by the caches.  48 B of own flow per pixel
//                       from memory, 6 + 24 + 1 = 31 B written.  No LDS, no atomics: nothing is shared between lanes.
// All three walk rows and images with grid-stride loops, so no size is limited by the grid's y and z extents.  Index arithmetic is 64-bit.
#pragma once

#define FP_TW 64
#define FP_TH 4
#define FP_THREADS (FP_TW * FP_TH)
#define FP_MAX_GRID_YZ 65535

// One axis of a warp coordinate: m = index + flow (already one rounded add), n = the image's extent along the axis.  The coordinate is clamped
// to [-2, (float)(n + 1)] (NaN -> -2): beyond either bound both taps are outside the image, so no result with a tap inside changes, and the
// integer conversions below are defined for every input.  -> i: the first tap, a: the weight of the second.
__device__ __forceinline__ void fp_axis(float m, int n, int subpixel, long& i, float& a) {
#pragma clang fp contract(off)
  const float hi = (float)((long)n + 1);
  m = m >= -2.f ? (m <= hi ? m : hi) : -2.f;
  if (subpixel) {  // OpenCV's fixed-point coordinates: 5 fractional bits, ties to even
    const long s = (long)rintf(m * 32.f);
    i = s >> 5;
    a = (float)(s & 31) / 32.f;
  } else {
    const float f = floorf(m);
    i = (long)f;
    a = m - f;
  }
}

struct FpCell {
  long o00, o01, o10, o11;  // pixel offsets of the four taps (rows of W pixels); valid where in*
  bool in00, in01, in10, in11;
  float w00, w01, w10, w11;
};

__device__ __forceinline__ FpCell fp_cell(int x, int y, float u, float v, int H, int W, int subpixel) {
#pragma clang fp contract(off)
  long ix, iy;
  float ax, ay;
  fp_axis((float)x + u, W, subpixel, ix, ax);
  fp_axis((float)y + v, H, subpixel, iy, ay);
  FpCell c;
  const bool x0 = ix >= 0 && ix < W, x1 = ix + 1 >= 0 && ix + 1 < W, y0 = iy >= 0 && iy < H, y1 = iy + 1 >= 0 && iy + 1 < H;
  c.in00 = x0 && y0; c.in01 = x1 && y0; c.in10 = x0 && y1; c.in11 = x1 && y1;
  c.o00 = iy * W + ix; c.o01 = c.o00 + 1; c.o10 = c.o00 + W; c.o11 = c.o10 + 1;
  const float bx = 1.f - ax, by = 1.f - ay;
  c.w00 = bx * by; c.w01 = ax * by; c.w10 = bx * ay; c.w11 = ax * ay;
  return c;
}

// a tap outside the image is 0.f (BORDER_CONSTANT), per tap: it is never read
__device__ __forceinline__ float fp_blend(const FpCell& c, float t00, float t01, float t10, float t11) {
#pragma clang fp contract(off)
  return ((t00 * c.w00 + t01 * c.w01) + t10 * c.w10) + t11 * c.w11;
}

struct FpResizeArgs {
  const float* src;  // [B, Hs, Ws, 2]
  float* dst;        // [B, Hd, Wd, 2]
  int B, Hs, Ws, Hd, Wd;
  double scale_x, scale_y;
  float ratio_u, ratio_v;
};

__global__ __launch_bounds__(IG_THREADS) void k_flow_resize(FpResizeArgs a) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * IG_THREADS + threadIdx.x;
  if (x >= a.Wd) return;
  const bool copy = a.Hs == a.Hd && a.Ws == a.Wd;
  float fx = (float)(((double)x + 0.5) * a.scale_x - 0.5);  // the taps of k_resize_linear_f32
  int sx = (int)floorf(fx);
  fx = fx - (float)sx;
  if (sx < 0) {
    sx = 0;
    fx = 0.f;
  }
  const bool edge = sx >= a.Ws - 1;
  if (edge) sx = a.Ws - 1;
  const float wx = 1.f - fx;
  for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
    const float* S = a.src + (long)b * a.Hs * a.Ws * 2;
    for (int y = blockIdx.y; y < a.Hd; y += gridDim.y) {
      float* o = a.dst + (((long)b * a.Hd + y) * a.Wd + x) * 2;
      if (copy) {
        const float* s = S + ((long)y * a.Ws + x) * 2;
        o[0] = s[0];
        o[1] = s[1];
        continue;
      }
      float fy = (float)(((double)y + 0.5) * a.scale_y - 0.5);
      const int sy = (int)floorf(fy);
      fy = fy - (float)sy;
      const float* r0 = S + (long)ig_clamp(sy, a.Hs - 1) * a.Ws * 2;
      const float* r1 = S + (long)ig_clamp(sy + 1, a.Hs - 1) * a.Ws * 2;
      for (int c = 0; c < 2; ++c) {
        float v0, v1;
        if (edge) {
          v0 = r0[(long)sx * 2 + c];
          v1 = r1[(long)sx * 2 + c];
        } else {
          v0 = r0[(long)sx * 2 + c] * wx + r0[(long)(sx + 1) * 2 + c] * fx;
          v1 = r1[(long)sx * 2 + c] * wx + r1[(long)(sx + 1) * 2 + c] * fx;
        }
        const float v = v0 * (1.f - fy) + v1 * fy;
        o[c] = v * (c == 0 ? a.ratio_u : a.ratio_v);
      }
    }
  }
}

struct FpWarpArgs {
  const float* img;   // [B, H, W, C]
  const float* flow;  // [B, H, W, 2]
  float* out;         // [B, H, W, C]
  int B, H, W, C, subpixel;
};

__global__ __launch_bounds__(FP_THREADS) void k_warp_flow(FpWarpArgs a) {
  const int x = blockIdx.x * FP_TW + (threadIdx.x & (FP_TW - 1));
  if (x >= a.W) return;
  const int C = a.C;
  const long plane = (long)a.H * a.W;
  for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
    const float* I = a.img + (long)b * plane * C;
    for (int y = blockIdx.y * FP_TH + (threadIdx.x / FP_TW); y < a.H; y += gridDim.y * FP_TH) {
      const long p = (long)b * plane + (long)y * a.W + x;
      const FpCell c = fp_cell(x, y, a.flow[2 * p], a.flow[2 * p + 1], a.H, a.W, a.subpixel);
      for (int k = 0; k < C; ++k) {
        const float t00 = c.in00 ? I[c.o00 * C + k] : 0.f, t01 = c.in01 ? I[c.o01 * C + k] : 0.f;
        const float t10 = c.in10 ? I[c.o10 * C + k] : 0.f, t11 = c.in11 ? I[c.o11 * C + k] : 0.f;
        a.out[p * C + k] = fp_blend(c, t00, t01, t10, t11);
      }
    }
  }
}

struct FpSupArgs {
  const float2* flows;   // [N, 6, H, W]
  const double* F;       // [N, 6, 9] or null
  unsigned char* masks;  // [N, 6, H, W]
  float* epi;            // [N, 6, H, W] or null
  unsigned char* motion; // [N, H, W] or null
  int N, H, W, subpixel, min_votes;
  float epi_thresh;
  double alpha1, alpha2;
};

// the forward-backward check of a flow vector f against the partner flow w warped to its pixel, in double from the fp32 values
__device__ __forceinline__ unsigned char fp_consistent(float2 f, float wu, float wv, double alpha1, double alpha2) {
#pragma clang fp contract(off)
  const double fu = (double)f.x, fv = (double)f.y, pu = (double)wu, pv = (double)wv;
  const double a = fu + pu, b = fv + pv;
  const double e = sqrt(a * a + b * b);
  const double t = alpha1 * (sqrt(fu * fu + fv * fv) + sqrt(pu * pu + pv * pv)) + alpha2;
  return e < t ? 1 : 0;  // (a comparison with NaN is false)
}

// the Sampson distance of (x, y) -> (x + u, y + v) under the row-major F, in double; 0 for a non-finite flow or a vanishing denominator
__device__ __forceinline__ float fp_sampson(const double* F, int col, int row, float2 f) {
#pragma clang fp contract(off)
  if (!(fabsf(f.x) <= FLT_MAX && fabsf(f.y) <= FLT_MAX)) return 0.f;
  const double x = (double)col, y = (double)row, x2 = x + (double)f.x, y2 = y + (double)f.y;
  const double l0 = (F[0] * x + F[1] * y) + F[2], l1 = (F[3] * x + F[4] * y) + F[5], l2 = (F[6] * x + F[7] * y) + F[8];
  const double m0 = (F[0] * x2 + F[3] * y2) + F[6], m1 = (F[1] * x2 + F[4] * y2) + F[7];
  const double r = (x2 * l0 + y2 * l1) + l2;
  const double den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  return den > 0.0 ? (float)(fabs(r) / sqrt(den)) : 0.f;
}

__global__ __launch_bounds__(FP_THREADS) void k_flow_supervision(FpSupArgs a) {
  const int x = blockIdx.x * FP_TW + (threadIdx.x & (FP_TW - 1));
  if (x >= a.W) return;
  const long plane = (long)a.H * a.W;
  for (int i = blockIdx.z; i < a.N; i += gridDim.z) {
    for (int y = blockIdx.y * FP_TH + (threadIdx.x / FP_TW); y < a.H; y += gridDim.y * FP_TH) {
      const long pix = (long)y * a.W + x;
      int votes = 0;
      for (int j = 0; j < 6; ++j) {
        const int o = j < 3 ? j + 1 : 2 - j;  // +1, +2, +3, -1, -2, -3
        const long at = ((long)i * 6 + j) * plane + pix;
        const long p = (long)i + o;
        unsigned char m = 0;
        float e = 0.f;
        if (p >= 0 && p < a.N) {
          const float2 f = a.flows[at];
          const float2* P = a.flows + (p * 6 + (j + 3) % 6) * plane;  // the partner: the flow of frame i + o back to frame i
          const FpCell c = fp_cell(x, y, f.x, f.y, a.H, a.W, a.subpixel);
          const float2 z = make_float2(0.f, 0.f);
          const float2 t00 = c.in00 ? P[c.o00] : z, t01 = c.in01 ? P[c.o01] : z, t10 = c.in10 ? P[c.o10] : z, t11 = c.in11 ? P[c.o11] : z;
          m = fp_consistent(f, fp_blend(c, t00.x, t01.x, t10.x, t11.x), fp_blend(c, t00.y, t01.y, t10.y, t11.y), a.alpha1, a.alpha2);
          if (a.F) {
            e = fp_sampson(a.F + ((long)i * 6 + j) * 9, x, y, f);
            votes += (m && e > a.epi_thresh) ? 1 : 0;  // on the stored fp32 value: a consumer can redo the vote from the maps
          }
        }
        a.masks[at] = m;
        if (a.epi) a.epi[at] = e;
      }
      if (a.motion) a.motion[(long)i * plane + pix] = votes >= a.min_votes ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static int fp_grid_rows(int H) {
  const int t = dyn_cdiv(H, FP_TH);
  return t < FP_MAX_GRID_YZ ? t : FP_MAX_GRID_YZ;
}
static int fp_grid_images(long n) { return (int)(n < FP_MAX_GRID_YZ ? n : FP_MAX_GRID_YZ); }

extern "C" int dyn_flow_resize(int B, int Hs, int Ws, int Hd, int Wd, const float* src, float* dst, void* stream) {
  const char* who = "dyn_flow_resize";
  DYN_REQUIRE(B >= 1, "%s: B=%d is unsupported (at least 1)", who, B);
  DYN_REQUIRE(Hs >= 1 && Ws >= 1 && Hd >= 1 && Wd >= 1 && (long)Hs * Ws < (1L << 31) && (long)Hd * Wd < (1L << 31),
              "%s: %d x %d -> %d x %d is unsupported (sizes >= 1, H*W < 2^31)", who, Hs, Ws, Hd, Wd);
  DYN_REQUIRE(src && dst && src != dst && vl_aligned(src, 4) && vl_aligned(dst, 4), "%s: src and dst are required, on 4 bytes, and must differ", who);
  FpResizeArgs a;
  a.src = src; a.dst = dst;
  a.B = B; a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.scale_x = ig_scale(Ws, Wd);
  a.scale_y = ig_scale(Hs, Hd);
  a.ratio_u = (float)((double)Wd / (double)Ws);
  a.ratio_v = (float)((double)Hd / (double)Hs);
  DYN_LAUNCH(DYN_K_FLOW_RESIZE, who, k_flow_resize, dim3(dyn_cdiv(Wd, IG_THREADS), fp_grid_images(Hd), fp_grid_images(B)), dim3(IG_THREADS), 0,
             (hipStream_t)stream, a);
  return 0;
}

extern "C" int dyn_warp_flow(int B, int H, int W, int C, const float* img, const float* flow, float* out, int subpixel, void* stream) {
  const char* who = "dyn_warp_flow";
  DYN_REQUIRE(B >= 1, "%s: B=%d is unsupported (at least 1)", who, B);
  DYN_REQUIRE(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "%s: %d x %d is unsupported (sizes >= 1, H*W < 2^31)", who, H, W);
  DYN_REQUIRE(C >= 1 && C <= 4, "%s: C=%d is unsupported (1..4)", who, C);
  DYN_REQUIRE(subpixel == 0 || subpixel == 32, "%s: subpixel=%d is unsupported (32: fixed-point coordinates, 0: exact coordinates)", who, subpixel);
  DYN_REQUIRE(img && flow && out && img != out && flow != out, "%s: img, flow and out are required; out must be neither input", who);
  DYN_REQUIRE(vl_aligned(img, 4) && vl_aligned(flow, 4) && vl_aligned(out, 4), "%s: img, flow and out must start on 4 bytes", who);
  FpWarpArgs a;
  a.img = img; a.flow = flow; a.out = out;
  a.B = B; a.H = H; a.W = W; a.C = C; a.subpixel = subpixel;
  DYN_LAUNCH(DYN_K_WARP_FLOW, who, k_warp_flow, dim3(dyn_cdiv(W, FP_TW), fp_grid_rows(H), fp_grid_images(B)), dim3(FP_THREADS), 0,
             (hipStream_t)stream, a);
  return 0;
}

extern "C" int dyn_flow_supervision(int N, int H, int W, const float* flows, const double* F, double alpha1, double alpha2, int subpixel,
                                    float epi_thresh, int min_votes, void* masks, float* epi, void* motion, void* stream) {
  const char* who = "dyn_flow_supervision";
  DYN_REQUIRE(N >= 1, "%s: N=%d is unsupported (at least 1 frame)", who, N);
  DYN_REQUIRE(H >= 1 && W >= 1 && (long)H * W < (1L << 31), "%s: %d x %d is unsupported (sizes >= 1, H*W < 2^31)", who, H, W);
  DYN_REQUIRE(subpixel == 0 || subpixel == 32, "%s: subpixel=%d is unsupported (32: fixed-point coordinates, 0: exact coordinates)", who, subpixel);
  DYN_REQUIRE(flows && masks, "%s: flows and masks are required", who);
  DYN_REQUIRE(vl_aligned(flows, 8) && (!F || vl_aligned(F, 8)) && (!epi || vl_aligned(epi, 4)),
              "%s: flows and F must start on 8 bytes, epi on 4", who);
  DYN_REQUIRE(F || (!epi && !motion), "%s: epi and motion need the fundamental matrices F", who);
  DYN_REQUIRE(alpha1 == alpha1 && alpha2 == alpha2 && epi_thresh == epi_thresh, "%s: alpha1, alpha2 or epi_thresh is not a number", who);
  FpSupArgs a;
  a.flows = reinterpret_cast<const float2*>(flows);
  a.F = F;
  a.masks = static_cast<unsigned char*>(masks);
  a.epi = epi;
  a.motion = static_cast<unsigned char*>(motion);
  a.N = N; a.H = H; a.W = W; a.subpixel = subpixel; a.min_votes = min_votes;
  a.epi_thresh = epi_thresh;
  a.alpha1 = alpha1; a.alpha2 = alpha2;
  DYN_LAUNCH(DYN_K_FLOW_SUPERVISION, who, k_flow_supervision, dim3(dyn_cdiv(W, FP_TW), fp_grid_rows(H), fp_grid_images(N)), dim3(FP_THREADS), 0,
             (hipStream_t)stream, a);
  return 0;
}
