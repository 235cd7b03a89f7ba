// Masked LPIPS of the evaluation loop (eval_nvidia.py:250-263 im2tensor, :289-291 the model, :402-457 its three calls per view): LPIPS v0.1,
// net = 'alex', model = 'net-lin', for one frame and up to 8 masks.  The features do not depend on the mask: they are computed once.
// Included at the end of dyn_encoder.hip.
//
// The contract (restated in torch on the CPU by tests/lpips_restatement.py):
//   1. Preparation is k_metrics_tile's, bit for bit: valid = ((r + g) + b > 1e-3f) from pred, a uint8 target is float(u8) / 255.0f, with
//      apply_valid both images times valid.  Then im2tensor, x / 0.5f - 1.0f, and the scaling layer (x - shift) / scale with
//      shift (-.030, -.088, -.188), scale (.458, .448, .450), all in fp32 without contraction.
//   2. torchvision's AlexNet `features`, zero padding, bias, tapped after each ReLU: conv 3 -> 64 k11 s4 p2 | max-pool 3 s2, conv 64 -> 192 k5 p2 |
//      max-pool 3 s2, conv 192 -> 384 k3 p1 | conv 384 -> 256 k3 p1 | conv 256 -> 256 k3 p1.
//   3. Per tap pixel n = f / (sqrt(sum_c f^2) + 1e-10) for both images, d_l[h, w] = sum_c lin_l[c] (n0 - n1)^2 (no bias; dropout is the identity).
//   4. A mask's channel 0 is resized to the tap's resolution by nearest neighbour, src = (dst * n_in) / n_out in integers;
//      S_l = sum d_l m_l, M_l = sum m_l.  The caller forms lpips = sum_l S_l / M_l (a tap with M_l = 0 contributes 0).
//      The script's `models` package is NSFF's modified copy of LPIPS; its masked form has not been seen: this is the package's stated form.
//
//   k_lpips_prep     both prepared, scaled images, channels-last with a zero fourth channel ([2, H, W, 4]: a pixel is one 16-byte load), and valid.
//   k_lpips_conv     implicit GEMM on the matrix pipe with v_mfma_f32_32x32x2_f32 -- true fp32 products, fp32 accumulate -- evaluated transposed like
//                    the encoder's: out^T [32 channels x 32 pixels] = W [32 x K] . patch^T [K x 32], K = (ky, kx, input channel).  One workgroup of four
//                    wavefronts owns one tile; the wavefronts split K in four contiguous runs and their accumulators are added through LDS in the
//                    fixed order ((w0 + w1) + (w2 + w3)) + bias, then ReLU.  Both images go in one launch: the pixel list is the flattened
//                    [2, Hout, Wout].  A lane fetches four consecutive input channels of one kernel tap of its own pixel (16 bytes, zero outside the
//                    map) and the matching 16 bytes of the packed weights per four MFMAs.
//   k_lpips_pool     max-pool 3 x 3 stride 2 (every window is full: H, W >= 31).
//   k_lpips_tap      a wavefront per tap pixel of all five taps: the two norms and d_l in double, butterfly sums over the lanes.
//   k_lpips_sums     per 256 tap pixels one row of partials [M][2] = (sum d m, sum m), every entry written.
//   k_lpips_finish   a workgroup per tap: the rows of that tap added in k_metrics_finish's fixed order.
//
// Arithmetic.  Features are fp32 (the products of the fp32 MFMA are not split: nothing to range-check beyond finiteness); from the norms on everything is
// double in a fixed order.  No atomics; nothing depends on the grid, the stream or M; a mask's sums do not depend on its neighbours; two calls give
// the same bits.  Identical images run the same operations on the same bits in both halves of every launch: every d_l is exactly 0.
#pragma once

#define LP_TAPS 5
#define LP_THREADS 256
#define LP_MAX_MASKS 8
#define LP_SUM_CHUNK 256  // tap pixels per row of partials

struct LpConvShape {
  int cin4, cout, k, stride, pad;  // cin4: input channels as stored (the image's three padded to four)
};
static constexpr LpConvShape LP_CONV[LP_TAPS] = {{4, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
static constexpr int LP_CIN[LP_TAPS] = {3, 64, 192, 384, 256};  // input channels of the state dict's tensors
// K in 16-byte slots (four channels of one tap), and in units of two slots (one per half of the wavefront = four MFMA steps)
constexpr int lp_slots(int l) { return LP_CONV[l].k * LP_CONV[l].k * LP_CONV[l].cin4 / 4; }
constexpr int lp_units(int l) { return (lp_slots(l) + 1) / 2; }
constexpr size_t lp_image_floats(int l) { return (size_t)(LP_CONV[l].cout / 32) * lp_units(l) * 256; }
constexpr size_t lp_off_conv(int l) { return l == 0 ? 0 : lp_off_conv(l - 1) + lp_image_floats(l - 1); }
constexpr size_t lp_off_bias(int l) { return l == 0 ? lp_off_conv(LP_TAPS - 1) + lp_image_floats(LP_TAPS - 1) : lp_off_bias(l - 1) + LP_CONV[l - 1].cout; }
constexpr size_t lp_off_lin(int l) { return l == 0 ? lp_off_bias(LP_TAPS - 1) + LP_CONV[LP_TAPS - 1].cout : lp_off_lin(l - 1) + LP_CONV[l - 1].cout; }
constexpr size_t LP_BLOB_FLOATS = lp_off_lin(LP_TAPS - 1) + LP_CONV[LP_TAPS - 1].cout;

extern "C" size_t dyn_lpips_blob_floats(void) { return LP_BLOB_FLOATS; }

// tensors: features.{0,3,6,8,10}.{weight,bias} (10, row-major [cout, cin, k, k] and [cout]), then lin{0..4} ([cout])
extern "C" int dyn_lpips_pack(const float* const* T, float* blob, size_t blob_floats) {
  DYN_REQUIRE(T && blob, "dyn_lpips_pack: null pointer");
  DYN_REQUIRE(blob_floats >= LP_BLOB_FLOATS, "dyn_lpips_pack: blob too small");
  for (int i = 0; i < 3 * LP_TAPS; ++i) DYN_REQUIRE(T[i] != nullptr, "dyn_lpips_pack: tensor %d is NULL", i);
  const size_t off_conv[LP_TAPS] = {lp_off_conv(0), lp_off_conv(1), lp_off_conv(2), lp_off_conv(3), lp_off_conv(4)};
  const size_t off_bias[LP_TAPS] = {lp_off_bias(0), lp_off_bias(1), lp_off_bias(2), lp_off_bias(3), lp_off_bias(4)};
  const size_t off_lin[LP_TAPS] = {lp_off_lin(0), lp_off_lin(1), lp_off_lin(2), lp_off_lin(3), lp_off_lin(4)};
  const int units[LP_TAPS] = {lp_units(0), lp_units(1), lp_units(2), lp_units(3), lp_units(4)};
  memset(blob, 0, LP_BLOB_FLOATS * sizeof(float));
  for (int l = 0; l < LP_TAPS; ++l) {
    const LpConvShape s = LP_CONV[l];
    const int cin = LP_CIN[l], cq = s.cin4 / 4, taps = s.k * s.k;
    const float *W = T[2 * l], *B = T[2 * l + 1], *L = T[2 * LP_TAPS + l];
    for (long i = 0; i < (long)s.cout * cin * taps; ++i)
      DYN_REQUIRE(fabsf(W[i]) <= 3.4028234663852886e38f, "dyn_lpips_pack: features weight %d has an element that is not finite", l);
    for (int c = 0; c < s.cout; ++c) {
      DYN_REQUIRE(fabsf(B[c]) <= 3.4028234663852886e38f, "dyn_lpips_pack: features bias %d has an element that is not finite", l);
      DYN_REQUIRE(L[c] >= 0.f && L[c] <= 3.4028234663852886e38f, "dyn_lpips_pack: lin%d has a negative or non-finite weight", l);
      blob[off_bias[l] + c] = B[c];
      blob[off_lin[l] + c] = L[c];
    }
    // image (t, u): 64 lanes x 4 floats; lane (n = lane & 31, h = lane >> 5), element j: W[32 t + n][slot 2 u + h][j], slot = tap * cq + channel quad
    float* img = blob + off_conv[l];
    for (int t = 0; t < s.cout / 32; ++t)
      for (int u = 0; u < units[l]; ++u)
        for (int lane = 0; lane < 64; ++lane) {
          const int oc = 32 * t + (lane & 31), slot = 2 * u + (lane >> 5);
          const int tap = slot / cq, c0 = (slot - tap * cq) * 4;
          for (int j = 0; j < 4; ++j) {
            const int c = c0 + j;
            img[((size_t)(t * units[l] + u) * 64 + lane) * 4 + j] = (tap < taps && c < cin) ? W[((size_t)oc * cin + c) * taps + tap] : 0.f;
          }
        }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double lp_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// one pixel per thread.  img4 [2][H][W][4] (pred, target; channel 3 = 0), valid [H][W] 1.f / 0.f, prepared (optional) [2][H][W][3]
__global__ __launch_bounds__(LP_THREADS) void k_lpips_prep(DynLpipsParams p, float* __restrict__ img4, float* __restrict__ valid) {
#pragma clang fp contract(off)
  const long pix = (long)blockIdx.x * LP_THREADS + threadIdx.x, hw = (long)p.H * p.W;
  if (pix >= hw) return;
  const float* pr = p.pred + pix * 3;
  float a[3] = {pr[0], pr[1], pr[2]}, b[3];
  const float v = ((a[0] + a[1]) + a[2] > 1e-3f) ? 1.f : 0.f;
  if (p.target_is_u8) {
    const unsigned char* tg = (const unsigned char*)p.target + pix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = (float)tg[c] / 255.0f;
  } else {
    const float* tg = (const float*)p.target + pix * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) b[c] = tg[c];
  }
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (p.apply_valid) {
      a[c] = a[c] * v;
      b[c] = b[c] * v;
    }
    a[c] = ((a[c] / 0.5f - 1.0f) - shift[c]) / scale[c];
    b[c] = ((b[c] / 0.5f - 1.0f) - shift[c]) / scale[c];
    if (p.prepared) {
      p.prepared[pix * 3 + c] = a[c];
      p.prepared[(hw + pix) * 3 + c] = b[c];
    }
  }
  reinterpret_cast<float4*>(img4)[pix] = make_float4(a[0], a[1], a[2], 0.f);
  reinterpret_cast<float4*>(img4)[hw + pix] = make_float4(b[0], b[1], b[2], 0.f);
  valid[pix] = v;
}

struct LpConvArgs {
  const float* in;    // [2][Hin][Win][CIN4]
  const float* wimg;  // packed images [COUT / 32][units][64 lanes][4]
  const float* bias;  // [COUT]
  float* out;         // [2][Hout][Wout][COUT], bias and ReLU applied
  int Hin, Win, Hout, Wout, cout;
};

#define LP_CONV_AHEAD 4  // units fetched ahead of the MFMAs that consume them

// grid (pixel tiles of the flattened [2, Hout, Wout], COUT / 32), block 256 = four wavefronts, each a contiguous quarter of the K units
template <int KS, int STRIDE, int PAD, int CIN4>
__global__ __launch_bounds__(LP_THREADS) void k_lpips_conv(LpConvArgs p) {
  constexpr int CQ = CIN4 / 4, TAPS = KS * KS, SLOTS = TAPS * CQ, UNITS = (SLOTS + 1) / 2;
  float (*red)[16][64] = reinterpret_cast<float (*)[16][64]>(dyn_smem);  // [4 waves][16 registers][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5, wave = tid >> 6;
  const long npix = 2L * p.Hout * p.Wout;
  long pix = (long)blockIdx.x * 32 + j;
  if (pix >= npix) pix = npix - 1;  // idle lanes shadow the last pixel (loads stay in bounds, nothing is stored)
  const int hw = p.Hout * p.Wout;
  const int n = (int)(pix / hw), rem = (int)(pix - (long)n * hw), oy = rem / p.Wout, ox = rem - oy * p.Wout;
  const float* inb = p.in + (long)n * p.Hin * p.Win * CIN4;
  const float4* wl = reinterpret_cast<const float4*>(p.wimg) + (size_t)blockIdx.y * UNITS * 64 + lane;
  const int iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
  const int u_lo = UNITS * wave / 4, u_hi = UNITS * (wave + 1) / 4;
  auto load_b = [&](int u) -> float4 {
    const int slot = 2 * u + h, tap = slot / CQ, cq = slot - tap * CQ, ky = tap / KS, kx = tap - ky * KS;
    const int iy = iy0 + ky, ix = ix0 + kx;
    if (slot >= SLOTS || iy < 0 || iy >= p.Hin || ix < 0 || ix >= p.Win) return make_float4(0.f, 0.f, 0.f, 0.f);
    return *reinterpret_cast<const float4*>(inb + ((long)iy * p.Win + ix) * CIN4 + cq * 4);
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float4 ra[LP_CONV_AHEAD], rb[LP_CONV_AHEAD];
#pragma unroll
  for (int i = 0; i < LP_CONV_AHEAD; ++i)
    if (u_lo + i < u_hi) {
      ra[i] = wl[(size_t)(u_lo + i) * 64];
      rb[i] = load_b(u_lo + i);
    }
  for (int u0 = u_lo; u0 < u_hi; u0 += LP_CONV_AHEAD) {
#pragma unroll
    for (int i = 0; i < LP_CONV_AHEAD; ++i) {
      const int u = u0 + i;
      if (u < u_hi) {  // (wave-uniform)
        const float4 a = ra[i], b = rb[i];
        if (u + LP_CONV_AHEAD < u_hi) {
          ra[i] = wl[(size_t)(u + LP_CONV_AHEAD) * 64];
          rb[i] = load_b(u + LP_CONV_AHEAD);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
  __syncthreads();
  // thread (q = wave, lane): registers 4 q .. 4 q + 3 of the lane's pixel = channels 8 q + 4 h + (0..3) of the tile
  if ((long)blockIdx.x * 32 + j < npix) {
    const int c0 = 32 * (int)blockIdx.y + 8 * wave + 4 * h;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * wave + e;
      const float s = ((red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane])) + p.bias[c0 + e];
      o[e] = fmaxf(s, 0.f);
    }
    *reinterpret_cast<float4*>(p.out + pix * p.cout + c0) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// in [2][Hin][Win][C] -> out [2][Hout][Wout][C], Hout = (Hin - 3) / 2 + 1; one thread per four channels of an output pixel
__global__ __launch_bounds__(LP_THREADS) void k_lpips_pool(const float* __restrict__ in, int Hin, int Win, int C, int Hout, int Wout,
                                                           float* __restrict__ out) {
  const int cq = C / 4;
  const long total = 2L * Hout * Wout * cq, idx = (long)blockIdx.x * LP_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % cq);
  const long pix = idx / cq;
  const int ox = (int)(pix % Wout), oy = (int)((pix / Wout) % Hout), n = (int)(pix / ((long)Wout * Hout));
  const float4* src = reinterpret_cast<const float4*>(in) + (((long)n * Hin + 2 * oy) * Win + 2 * ox) * cq + q;
  float4 m = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 v = src[((long)dy * Win + dx) * cq];
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  reinterpret_cast<float4*>(out)[idx] = m;
}

struct LpTaps {
  const float* feat[LP_TAPS];  // [2][Hl][Wl][C_l]
  const float* lin[LP_TAPS];   // [C_l]
  int Hl[LP_TAPS], Wl[LP_TAPS], C[LP_TAPS];
  long first[LP_TAPS + 1];     // first tap pixel of tap l in the list of all tap pixels
};

// a wavefront per tap pixel; lane l holds channels l, l + 64, ... (at most 6: C <= 384).  dmap [first[5]] doubles, maps: the caller's copy or NULL
__global__ __launch_bounds__(LP_THREADS) void k_lpips_tap(LpTaps t, double* __restrict__ dmap, double* __restrict__ maps) {
  const int lane = dyn_lane();
  const long pix = (long)blockIdx.x * (LP_THREADS / 64) + dyn_wave();
  if (pix >= t.first[LP_TAPS]) return;
  int l = 0;
#pragma unroll
  for (int i = 1; i < LP_TAPS; ++i) l += pix >= t.first[i] ? 1 : 0;
  const int C = t.C[l];
  const long local = pix - t.first[l], hw = (long)t.Hl[l] * t.Wl[l];
  const float *f0 = t.feat[l] + local * C, *f1 = t.feat[l] + (hw + local) * C, *lin = t.lin[l];
  double x0[6], x1[6], s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int c = lane + 64 * i;
    x0[i] = c < C ? (double)f0[c] : 0.0;
    x1[i] = c < C ? (double)f1[c] : 0.0;
    s0 += x0[i] * x0[i];
    s1 += x1[i] * x1[i];
  }
  const double r0 = sqrt(lp_wave_sum(s0)) + 1e-10, r1 = sqrt(lp_wave_sum(s1)) + 1e-10;
  double d = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int c = lane + 64 * i;
    const double e = x0[i] / r0 - x1[i] / r1;
    d += c < C ? (double)lin[c] * (e * e) : 0.0;
  }
  d = lp_wave_sum(d);
  if (lane == 0) {
    dmap[pix] = d;
    if (maps) maps[pix] = d;
  }
}

struct LpMasks {
  const float* valid;  // [H][W] of k_lpips_prep
  const float* masks;
  long mask_stride;
  int mask_channels, valid_as_mask0, M, H, W;
};
__host__ __device__ inline long lp_rows_of(long npix) { return (npix + LP_SUM_CHUNK - 1) / LP_SUM_CHUNK; }

// grid: the rows of all taps (tap after tap, row_first[l] the first row of tap l); partial [rows][M][2] = (sum d m, sum m) of the row's pixels
__global__ __launch_bounds__(LP_SUM_CHUNK) void k_lpips_sums(LpTaps t, LpMasks k, const double* __restrict__ dmap, double* __restrict__ partial) {
  double (*red)[LP_SUM_CHUNK / 64] = reinterpret_cast<double (*)[LP_SUM_CHUNK / 64]>(dyn_smem);  // [2 M][waves]
  const int tid = threadIdx.x, lane = dyn_lane(), wave = dyn_wave();
  long row = blockIdx.x;
  int l = 0;
  for (; l < LP_TAPS - 1; ++l) {
    const long r = lp_rows_of(t.first[l + 1] - t.first[l]);
    if (row < r) break;
    row -= r;
  }
  const long local = row * LP_SUM_CHUNK + tid, hw = (long)t.Hl[l] * t.Wl[l];
  const bool in = local < hw;
  double d = 0.0;
  long src = 0;
  if (in) {
    const int y = (int)(local / t.Wl[l]), x = (int)(local - (long)y * t.Wl[l]);
    const int sy = (int)(((long)y * k.H) / t.Hl[l]), sx = (int)(((long)x * k.W) / t.Wl[l]);
    src = (long)sy * k.W + sx;
    d = dmap[t.first[l] + local];
  }
  for (int m = 0; m < k.M; ++m) {
    double w = 0.0;
    if (in) {
      if (k.valid_as_mask0 && m == 0) w = (double)k.valid[src];
      else w = (double)k.masks[(long)(m - (k.valid_as_mask0 ? 1 : 0)) * k.mask_stride + src * k.mask_channels];
    }
    const double s = lp_wave_sum(d * w), c = lp_wave_sum(w);
    if (lane == 0) {
      red[2 * m][wave] = s;
      red[2 * m + 1][wave] = c;
    }
  }
  __syncthreads();
  if (tid < k.M * 2) partial[(long)blockIdx.x * (k.M * 2) + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// grid LP_TAPS: sums [M][5][2] <- the columns of the tap's rows, each added by one wavefront in k_metrics_finish's order
__global__ __launch_bounds__(LP_THREADS) void k_lpips_finish(LpTaps t, int M, const double* __restrict__ partial, double* __restrict__ sums) {
  const int lane = dyn_lane(), wave = dyn_wave(), l = blockIdx.x, ncol = M * 2;
  long row0 = 0;
  for (int i = 0; i < l; ++i) row0 += lp_rows_of(t.first[i + 1] - t.first[i]);
  const long rows = lp_rows_of(t.first[l + 1] - t.first[l]);
  const double* part = partial + row0 * ncol;
  for (int k = wave; k < ncol; k += LP_THREADS / 64) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    long i = lane;
    for (; i + 192 < rows; i += 256) {
      s0 += part[i * ncol + k];
      s1 += part[(i + 64) * ncol + k];
      s2 += part[(i + 128) * ncol + k];
      s3 += part[(i + 192) * ncol + k];
    }
    if (i < rows) s0 += part[i * ncol + k];
    if (i + 64 < rows) s1 += part[(i + 64) * ncol + k];
    if (i + 128 < rows) s2 += part[(i + 128) * ncol + k];
    const double v = lp_wave_sum((s0 + s1) + (s2 + s3));
    if (lane == 0) sums[((long)(k >> 1) * LP_TAPS + l) * 2 + (k & 1)] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
struct LpWs {
  int Hf[LP_TAPS], Wf[LP_TAPS];  // the taps
  int Hp[2], Wp[2];              // the two pooled maps
  long first[LP_TAPS + 1], rows;
  size_t off_img, off_valid, off_feat[LP_TAPS], off_pool[2], off_dmap, off_partial, total;  // bytes
};
static bool lp_shape_ok(int H, int W, int M) { return H >= 31 && W >= 31 && (long)H * W * 4 < (1L << 31) && M >= 1 && M <= LP_MAX_MASKS; }
static LpWs lp_ws(int H, int W, int M) {
  LpWs w;
  w.Hf[0] = (H + 4 - 11) / 4 + 1; w.Wf[0] = (W + 4 - 11) / 4 + 1;
  w.Hp[0] = (w.Hf[0] - 3) / 2 + 1; w.Wp[0] = (w.Wf[0] - 3) / 2 + 1;
  w.Hf[1] = w.Hp[0]; w.Wf[1] = w.Wp[0];
  w.Hp[1] = (w.Hf[1] - 3) / 2 + 1; w.Wp[1] = (w.Wf[1] - 3) / 2 + 1;
  for (int l = 2; l < LP_TAPS; ++l) { w.Hf[l] = w.Hp[1]; w.Wf[l] = w.Wp[1]; }
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  w.off_img = take((size_t)2 * H * W * 4 * sizeof(float));
  w.off_valid = take((size_t)H * W * sizeof(float));
  w.first[0] = 0;
  w.rows = 0;
  for (int l = 0; l < LP_TAPS; ++l) {
    w.off_feat[l] = take((size_t)2 * w.Hf[l] * w.Wf[l] * LP_CONV[l].cout * sizeof(float));
    w.first[l + 1] = w.first[l] + (long)w.Hf[l] * w.Wf[l];
    w.rows += lp_rows_of((long)w.Hf[l] * w.Wf[l]);
  }
  for (int i = 0; i < 2; ++i) w.off_pool[i] = take((size_t)2 * w.Hp[i] * w.Wp[i] * LP_CONV[i].cout * sizeof(float));
  w.off_dmap = take((size_t)w.first[LP_TAPS] * sizeof(double));
  w.off_partial = take((size_t)w.rows * M * 2 * sizeof(double));
  w.total = o;
  return w;
}

extern "C" size_t dyn_lpips_workspace_bytes(int H, int W, int M) { return lp_shape_ok(H, W, M) ? lp_ws(H, W, M).total : 0; }
extern "C" long dyn_lpips_map_doubles(int H, int W) { return lp_shape_ok(H, W, 1) ? lp_ws(H, W, 1).first[LP_TAPS] : 0; }

template <int L>
static int lp_launch_conv(const DynLpipsParams* p, const float* in, int Hin, int Win, float* out, int Hout, int Wout, hipStream_t st) {
  constexpr LpConvShape s = LP_CONV[L];
  const LpConvArgs a{in, p->blob + lp_off_conv(L), p->blob + lp_off_bias(L), out, Hin, Win, Hout, Wout, s.cout};
  const dim3 grid((unsigned)dyn_cdiv(2L * Hout * Wout, 32), s.cout / 32);
  DYN_LAUNCH(DYN_K_LPIPS_CONV, "k_lpips_conv", (k_lpips_conv<s.k, s.stride, s.pad, s.cin4>), grid, dim3(LP_THREADS), 4 * 16 * 64 * sizeof(float), st, a);
  return 0;
}

extern "C" int dyn_lpips_frame(const DynLpipsParams* p, double* sums, void* stream) {
  DYN_REQUIRE(p, "dyn_lpips_frame: null params");
  DYN_REQUIRE(p->H >= 31 && p->W >= 31, "dyn_lpips_frame: H=%d W=%d is smaller than 31 x 31 (both max-pools need a full window)", p->H, p->W);
  DYN_REQUIRE((long)p->H * p->W * 4 < (1L << 31), "dyn_lpips_frame: H=%d W=%d is too large (H*W*4 < 2^31)", p->H, p->W);
  DYN_REQUIRE(p->M >= 1 && p->M <= LP_MAX_MASKS, "dyn_lpips_frame: M=%d masks (1..%d)", p->M, LP_MAX_MASKS);
  DYN_REQUIRE(p->blob && p->pred && p->target && sums, "dyn_lpips_frame: blob, pred, target and sums are required");
  const int user_masks = p->M - (p->valid_as_mask0 ? 1 : 0);
  DYN_REQUIRE(user_masks == 0 || p->masks, "dyn_lpips_frame: masks is required for M=%d", p->M);
  DYN_REQUIRE(user_masks == 0 || p->mask_channels == 1 || p->mask_channels == 3, "dyn_lpips_frame: mask_channels=%d (1 or 3)", p->mask_channels);
  DYN_REQUIRE(user_masks <= 1 || p->mask_stride >= (long)p->H * p->W * p->mask_channels, "dyn_lpips_frame: mask_stride=%ld is smaller than one mask",
              p->mask_stride);
  const LpWs w = lp_ws(p->H, p->W, p->M);
  DYN_REQUIRE(p->workspace && p->workspace_bytes >= w.total, "dyn_lpips_frame: workspace of %zu bytes given, %zu needed", p->workspace_bytes, w.total);
  DYN_REQUIRE(((uintptr_t)p->workspace & 15) == 0 && ((uintptr_t)p->blob & 15) == 0, "dyn_lpips_frame: workspace and blob must be 16-byte aligned");
  DYN_REQUIRE(((uintptr_t)sums & 7) == 0 && ((uintptr_t)p->maps & 7) == 0, "dyn_lpips_frame: sums and maps must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)p->workspace;
  float *img4 = (float*)(ws + w.off_img), *valid = (float*)(ws + w.off_valid);
  float* feat[LP_TAPS];
  for (int l = 0; l < LP_TAPS; ++l) feat[l] = (float*)(ws + w.off_feat[l]);
  float* pool[2] = {(float*)(ws + w.off_pool[0]), (float*)(ws + w.off_pool[1])};
  double *dmap = (double*)(ws + w.off_dmap), *partial = (double*)(ws + w.off_partial);
  int rc;
  DYN_LAUNCH(DYN_K_LPIPS_PREP, "k_lpips_prep", k_lpips_prep, dim3((unsigned)dyn_cdiv((long)p->H * p->W, LP_THREADS)), dim3(LP_THREADS), 0, st, *p, img4, valid);
  if ((rc = lp_launch_conv<0>(p, img4, p->H, p->W, feat[0], w.Hf[0], w.Wf[0], st))) return rc;
  DYN_LAUNCH(DYN_K_LPIPS_POOL, "k_lpips_pool", k_lpips_pool, dim3((unsigned)dyn_cdiv(2L * w.Hp[0] * w.Wp[0] * 16, LP_THREADS)), dim3(LP_THREADS), 0, st,
             (const float*)feat[0], w.Hf[0], w.Wf[0], 64, w.Hp[0], w.Wp[0], pool[0]);
  if ((rc = lp_launch_conv<1>(p, pool[0], w.Hp[0], w.Wp[0], feat[1], w.Hf[1], w.Wf[1], st))) return rc;
  DYN_LAUNCH(DYN_K_LPIPS_POOL, "k_lpips_pool", k_lpips_pool, dim3((unsigned)dyn_cdiv(2L * w.Hp[1] * w.Wp[1] * 48, LP_THREADS)), dim3(LP_THREADS), 0, st,
             (const float*)feat[1], w.Hf[1], w.Wf[1], 192, w.Hp[1], w.Wp[1], pool[1]);
  if ((rc = lp_launch_conv<2>(p, pool[1], w.Hp[1], w.Wp[1], feat[2], w.Hf[2], w.Wf[2], st))) return rc;
  if ((rc = lp_launch_conv<3>(p, feat[2], w.Hf[2], w.Wf[2], feat[3], w.Hf[3], w.Wf[3], st))) return rc;
  if ((rc = lp_launch_conv<4>(p, feat[3], w.Hf[3], w.Wf[3], feat[4], w.Hf[4], w.Wf[4], st))) return rc;
  LpTaps t;
  const size_t off_lin[LP_TAPS] = {lp_off_lin(0), lp_off_lin(1), lp_off_lin(2), lp_off_lin(3), lp_off_lin(4)};
  for (int l = 0; l < LP_TAPS; ++l) {
    t.feat[l] = feat[l];
    t.lin[l] = p->blob + off_lin[l];
    t.Hl[l] = w.Hf[l]; t.Wl[l] = w.Wf[l]; t.C[l] = LP_CONV[l].cout;
    t.first[l] = w.first[l];
  }
  t.first[LP_TAPS] = w.first[LP_TAPS];
  const LpMasks k{valid, p->masks, p->mask_stride, p->mask_channels, p->valid_as_mask0 ? 1 : 0, p->M, p->H, p->W};
  DYN_LAUNCH(DYN_K_LPIPS_TAP, "k_lpips_tap", k_lpips_tap, dim3((unsigned)dyn_cdiv(w.first[LP_TAPS], LP_THREADS / 64)), dim3(LP_THREADS), 0, st, t, dmap, p->maps);
  DYN_LAUNCH(DYN_K_LPIPS_SUMS, "k_lpips_sums", k_lpips_sums, dim3((unsigned)w.rows), dim3(LP_SUM_CHUNK),
             LP_MAX_MASKS * 2 * (LP_SUM_CHUNK / 64) * sizeof(double), st, t, k, (const double*)dmap, partial);
  DYN_LAUNCH(DYN_K_LPIPS_FINISH, "k_lpips_finish", k_lpips_finish, dim3(LP_TAPS), dim3(LP_THREADS), 0, st, t, p->M, (const double*)partial, sums);
  return 0;
}
