// Frame metrics of the evaluation loop (eval_nvidia.py:201-247, :383-457 without LPIPS): the valid mask and the prepared images, the SSIM
// map of skimage.metrics.structural_similarity as eval_nvidia.py:242-244 calls it (defaults, channel axis last, full=True), and for each
// of M masks the three sums the script's calculate_psnr / calculate_ssim divide: sum((a - b)^2 m), sum(S m), sum(m).
// Included from dyn_geometry.hip: the unit is built with -ffp-contract=off, which the bitwise contract of the preparation needs.
//
//   k_metrics_tile     one workgroup per tile of 32 x 8 pixels.  The tile and a 3-pixel halo of both prepared images go to LDS as fp32,
//                      scipy's `reflect` boundary (d c b a | a b c d) applied to the indices while loading.  Preparation per loaded pixel
//                      (:383-396): valid = ((r + g) + b > 1e-3f) in fp32 in numpy's order of addition, a uint8 target becomes
//                      float(u8) / 255.0f (a correctly rounded fp32 division), both images are multiplied by valid.  Each thread then
//                      forms the five 7 x 7 window sums of its pixel per channel straight from LDS, S, and its contribution to the
//                      3 M sums; the workgroup's sums are stored as one row of partials (plain stores, every entry written).
//   k_metrics_finish   one workgroup, a wavefront per column of partials: lane l adds the rows l, l + 64, ... in ascending order, the 64
//                      lane sums are combined by a fixed butterfly -- the same order in every call (k_objective_finish's scheme).
//
// Arithmetic.  Everything that is a sum or a cancellation is double: the products x*x, y*y, x*y of fp32 values are exact in double, the
// 49-term window sums run in row-major window order, then u = sum / 49, v = (49 / 48) (uxx - ux ux), C1 = (0.01 R)^2, C2 = (0.03 R)^2,
// S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)).  With identical images numerator and denominator are the same
// operations on the same bits, so S is exactly 1.  No float atomics, no order that depends on the grid or the stream: a mask's sums depend
// on the frame and that mask alone (not on M), and two calls give the same bits.
// The frame is 0.44 M values and every input stays in the caches: a latency- and launch-bound pair of kernels.
#pragma once

#define MET_TW 32
#define MET_TH 8
#define MET_THREADS (MET_TW * MET_TH)
#define MET_PAD 3                               // (win_size - 1) / 2 of the 7 x 7 window
#define MET_LW (MET_TW + 2 * MET_PAD)           // 38
#define MET_LH (MET_TH + 2 * MET_PAD)           // 14
#define MET_PLANE (MET_LW * MET_LH)             // floats per channel plane of one image
#define MET_LDS_IMG (2 * 3 * MET_PLANE * 4)     // bytes: both images, three planes each
#define MET_MAX_MASKS 8
#define MET_FINISH_THREADS 256

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// scipy.ndimage's `reflect` (= numpy's `symmetric`): -1 -> 0, -2 -> 1, n -> n - 1.  One reflection suffices inside the halo of an image with
// n >= 7; positions further out belong to threads beyond the image, which contribute nothing: they are clamped to stay inside the arrays.
__device__ __forceinline__ int met_reflect(int i, int n) {
  if (i < 0) i = -1 - i;
  if (i >= n) i = 2 * n - 1 - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

struct MetPixel {
  float a[3], b[3];  // prepared pred, prepared target
  float valid;       // 1.f / 0.f
};
__device__ __forceinline__ MetPixel met_prepare(const DynFrameMetricsParams& p, long pix) {
  MetPixel q;
  const float* pr = p.pred + pix * 3;
  const float r = pr[0], g = pr[1], b = pr[2];
  q.valid = ((r + g) + b > 1e-3f) ? 1.f : 0.f;  // np.sum(rgb, -1) > 1e-3 on float32 (:383-385)
  float t[3];
  if (p.target_is_u8) {
    const unsigned char* tg = (const unsigned char*)p.target + pix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = (float)tg[c] / 255.0f;  // np.float32(img) / 255 (:393)
  } else {
    const float* tg = (const float*)p.target + pix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = tg[c];
  }
  q.a[0] = r; q.a[1] = g; q.a[2] = b;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    q.b[c] = t[c];
    if (p.apply_valid) {  // (:395-396)
      q.a[c] = q.a[c] * q.valid;
      q.b[c] = q.b[c] * q.valid;
    }
  }
  return q;
}

// grid: tiles_x * tiles_y workgroups (1-D), block MET_THREADS.  partial [tiles][M][3] = (sum (a - b)^2 m, sum S m, sum m) of the tile.
__global__ __launch_bounds__(MET_THREADS) void k_metrics_tile(DynFrameMetricsParams p, int tiles_x, double* __restrict__ partial) {
  float* sa = reinterpret_cast<float*>(dyn_smem);  // [3][MET_LH][MET_LW]
  float* sb = sa + 3 * MET_PLANE;
  double* red = reinterpret_cast<double*>(sb + 3 * MET_PLANE);  // [M * 3][waves]
  const int tid = threadIdx.x, lane = dyn_lane(), wave = dyn_wave();
  const int ty0 = ((int)blockIdx.x / tiles_x) * MET_TH, tx0 = ((int)blockIdx.x % tiles_x) * MET_TW;
  for (int e = tid; e < MET_PLANE; e += MET_THREADS) {
    const int ly = e / MET_LW, lx = e - ly * MET_LW;
    const int gy = met_reflect(ty0 + ly - MET_PAD, p.H), gx = met_reflect(tx0 + lx - MET_PAD, p.W);
    const MetPixel q = met_prepare(p, (long)gy * p.W + gx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sa[c * MET_PLANE + e] = q.a[c];
      sb[c * MET_PLANE + e] = q.b[c];
    }
  }
  __syncthreads();
  const int lx = tid % MET_TW, ly = tid / MET_TW;
  const int gx = tx0 + lx, gy = ty0 + ly;
  const bool in = gx < p.W && gy < p.H;
  const long pix = (long)gy * p.W + gx;
  const int centre = (ly + MET_PAD) * MET_LW + lx + MET_PAD;
  const double R = p.data_range;
  const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R), cov_norm = 49.0 / 48.0;
  double S[3], d2[3];
  float valid = 0.f;
  if (in) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* xa = sa + c * MET_PLANE + ly * MET_LW + lx;
      const float* xb = sb + c * MET_PLANE + ly * MET_LW + lx;
      double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
      for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 7; ++dx) {
          const double x = (double)xa[dy * MET_LW + dx], y = (double)xb[dy * MET_LW + dx];
          sx += x;
          sy += y;
          sxx += x * x;
          syy += y * y;
          sxy += x * y;
        }
      }
      const double ux = sx / 49.0, uy = sy / 49.0, uxx = sxx / 49.0, uyy = syy / 49.0, uxy = sxy / 49.0;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      S[c] = (A1 * A2) / (B1 * B2);
      const float a = sa[c * MET_PLANE + centre], b = sb[c * MET_PLANE + centre];
      const double d = (double)a - (double)b;
      d2[c] = d * d;
      if (p.ssim_map) p.ssim_map[pix * 3 + c] = S[c];
      if (p.pred_out) p.pred_out[pix * 3 + c] = a;
      if (p.target_out) p.target_out[pix * 3 + c] = b;
    }
    const float* pr = p.pred + pix * 3;
    valid = ((pr[0] + pr[1]) + pr[2] > 1e-3f) ? 1.f : 0.f;
    if (p.valid) p.valid[pix] = valid != 0.f ? 1 : 0;
  }
  constexpr int NW = MET_THREADS / DYN_WAVE;
  for (int m = 0; m < p.M; ++m) {
    double e = 0.0, s = 0.0, n = 0.0;
    if (in) {
      float w[3];
      if (p.valid_as_mask0 && m == 0) {
        w[0] = w[1] = w[2] = valid;
      } else {
        const float* mk = p.masks + (long)(m - (p.valid_as_mask0 ? 1 : 0)) * p.mask_stride + pix * p.mask_channels;
        w[0] = mk[0];
        w[1] = p.mask_channels == 3 ? mk[1] : w[0];
        w[2] = p.mask_channels == 3 ? mk[2] : w[0];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double wc = (double)w[c];
        e += d2[c] * wc;
        s += S[c] * wc;
        n += wc;
      }
    }
    e = met_wave_sum(e);
    s = met_wave_sum(s);
    n = met_wave_sum(n);
    if (lane == 0) {
      red[(m * 3 + 0) * NW + wave] = e;
      red[(m * 3 + 1) * NW + wave] = s;
      red[(m * 3 + 2) * NW + wave] = n;
    }
  }
  __syncthreads();
  if (tid < p.M * 3) {
    double v = red[tid * NW];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += red[tid * NW + w];
    partial[(long)blockIdx.x * (p.M * 3) + tid] = v;
  }
}

// sums [M][3] <- the columns of partial [rows][ncol], each added by one wavefront in a fixed order
__global__ __launch_bounds__(MET_FINISH_THREADS) void k_metrics_finish(const double* __restrict__ partial, long rows, int ncol,
                                                                        double* __restrict__ sums) {
  const int lane = dyn_lane(), wave = dyn_wave();
  for (int k = wave; k < ncol; k += MET_FINISH_THREADS / DYN_WAVE) {
    // lane l adds rows l, l + 64, ... in ascending order into four accumulators (row / 64 mod 4: four loads in flight), then
    // ((s0 + s1) + (s2 + s3)) and the butterfly over the lanes
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long i = lane;
    for (; i + 192 < rows; i += 256) {
      s0 += partial[i * ncol + k];
      s1 += partial[(i + 64) * ncol + k];
      s2 += partial[(i + 128) * ncol + k];
      s3 += partial[(i + 192) * ncol + k];
    }
    if (i < rows) s0 += partial[i * ncol + k];
    if (i + 64 < rows) s1 += partial[(i + 64) * ncol + k];
    if (i + 128 < rows) s2 += partial[(i + 128) * ncol + k];
    const double v = met_wave_sum((s0 + s1) + (s2 + s3));
    if (lane == 0) sums[k] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static bool met_shape_ok(int H, int W, int M) {
  return H >= 7 && W >= 7 && (long)H * W * 3 < (1L << 31) && M >= 1 && M <= MET_MAX_MASKS;
}
static long met_tiles(int H, int W) { return (long)dyn_cdiv(H, MET_TH) * dyn_cdiv(W, MET_TW); }

extern "C" size_t dyn_frame_metrics_workspace_bytes(int H, int W, int M) {
  return met_shape_ok(H, W, M) ? (size_t)met_tiles(H, W) * M * 3 * sizeof(double) : 0;
}

extern "C" int dyn_frame_metrics(const DynFrameMetricsParams* p, double* sums, void* stream) {
  DYN_REQUIRE(p, "dyn_frame_metrics: null params");
  DYN_REQUIRE(p->H >= 7 && p->W >= 7, "dyn_frame_metrics: H=%d W=%d is smaller than the 7 x 7 window", p->H, p->W);
  DYN_REQUIRE((long)p->H * p->W * 3 < (1L << 31), "dyn_frame_metrics: H=%d W=%d is too large (H*W*3 < 2^31)", p->H, p->W);
  DYN_REQUIRE(p->M >= 1 && p->M <= MET_MAX_MASKS, "dyn_frame_metrics: M=%d masks (1..%d)", p->M, MET_MAX_MASKS);
  DYN_REQUIRE(p->data_range > 0.0 && p->data_range <= 1.7976931348623157e308, "dyn_frame_metrics: data_range must be positive and finite");
  DYN_REQUIRE(p->pred && p->target && sums, "dyn_frame_metrics: pred, target and sums are required");
  const int user_masks = p->M - (p->valid_as_mask0 ? 1 : 0);
  DYN_REQUIRE(user_masks == 0 || p->masks, "dyn_frame_metrics: masks is required for M=%d", p->M);
  DYN_REQUIRE(user_masks == 0 || p->mask_channels == 1 || p->mask_channels == 3, "dyn_frame_metrics: mask_channels=%d (1 or 3)",
              p->mask_channels);
  DYN_REQUIRE(user_masks <= 1 || p->mask_stride >= (long)p->H * p->W * p->mask_channels,
              "dyn_frame_metrics: mask_stride=%ld is smaller than one mask", p->mask_stride);
  const size_t need = dyn_frame_metrics_workspace_bytes(p->H, p->W, p->M);
  DYN_REQUIRE(p->workspace && p->workspace_bytes >= need, "dyn_frame_metrics: workspace of %zu bytes given, %zu needed", p->workspace_bytes,
              need);
  DYN_REQUIRE(((uintptr_t)p->workspace & 7) == 0 && ((uintptr_t)sums & 7) == 0, "dyn_frame_metrics: workspace and sums must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = dyn_cdiv(p->W, MET_TW);
  const long tiles = met_tiles(p->H, p->W);
  double* partial = (double*)p->workspace;
  const size_t lds = MET_LDS_IMG + (size_t)p->M * 3 * (MET_THREADS / DYN_WAVE) * sizeof(double);
  DYN_LAUNCH(DYN_K_METRICS_TILE, "k_metrics_tile", k_metrics_tile, dim3((unsigned)tiles), dim3(MET_THREADS), lds, st, *p, tiles_x, partial);
  DYN_LAUNCH(DYN_K_METRICS_FINISH, "k_metrics_finish", k_metrics_finish, dim3(1), dim3(MET_FINISH_THREADS), 0, st, (const double*)partial,
             tiles, p->M * 3, sums);
  return 0;
}
