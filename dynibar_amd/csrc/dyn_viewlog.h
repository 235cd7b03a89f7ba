// The view panels the training loop logs (train.py:576-762 log_view_to_tb, utils.py:97-170 colorize, flow_utils.py:17-153 flow_to_image)
// from the device-resident groups of a rendered frame: three launches, nothing through the host in between.
// Included from dyn_geometry.hip: -ffp-contract=off.  numpy and matplotlib do this arithmetic one operation at a time, most of it in
// double, and the panels are compared with theirs bit for bit: no product may be fused into a sum here (the one fused chain, the
// magnitude, is written with fmaf because torch.norm's host loop is that chain).
//
//   k_viewlog_ranges    one workgroup of 1024 threads per scalar image (a frame is 147 456 values = 0.6 MB and stays in L2: the kernel
//                       waits for loads, not for bandwidth).  An image given as [H,W,3] is first reduced to its magnitude
//                       sqrtf(fmaf(z, z, fmaf(y, y, x * x))) into the caller's buffer, which the passes then read.  colorize takes
//                       np.percentile(x, (1, 99)): two pairs of neighbouring order statistics.  The four ranks are selected EXACTLY by
//                       a radix select over the order-preserving key of the float (sign bit flipped for x >= 0, all bits for x < 0;
//                       -0.0 counts as +0.0, as it compares): pass 1 counts the top 11 bits of every key into one LDS histogram,
//                       passes 2 and 3 count the next 11 and the last 10 bits of the keys that share a rank's prefix, one histogram
//                       per rank (the prefixes of the four ranks part ways).  After each pass a scan over the 2048 bins -- 256 threads
//                       per rank, 8 bins each, shuffles within a wavefront and four wavefront totals through LDS -- finds the bin
//                       that holds the rank and the rank within that bin.  Integer counts only: the result does not depend on any
//                       order.  Then numpy's _lerp per percentile, see dyn_viewlog_ranges in the header.
//   k_viewlog_flow_max  grid (tiles, F): fp32 sqrtf(u*u + v*v) per pixel after the unknown-flow zeroing, the maximum over a wavefront by
//                       shuffles and one integer atomicMax on the bits per wavefront (non-negative floats order like their bits).
//   k_viewlog_panels    grid (tiles of 256 pixels, panels): a thread writes the three values of its pixel of its panel.
#pragma once

#define VL_THREADS 1024
#define VL_BINS 2048
#define VL_MAX_IMAGES 4
#define VL_MAX_FLOWS 12
#define VL_MAX_RGB 8
#define VL_TILE 256
#define VL_RANGES_LDS ((4 * VL_BINS + 16 + 8) * 4)

struct VlRangesArgs {
  const float* image[VL_MAX_IMAGES];
  float* mag_out[VL_MAX_IMAGES];
  int magnitude[VL_MAX_IMAGES];
  unsigned rank[4];
  double weight[2];
  long n;
  double* ranges;
};
struct VlFlowArgs {
  const float* flow[VL_MAX_FLOWS];
  long n;
};
struct VlPanelArgs {
  int n_rgb, n_map, n_flow, map_chw, flow_u8;
  long n;
  const float* rgb_src[VL_MAX_RGB];
  float* rgb_dst[VL_MAX_RGB];
  int rgb_clamp[VL_MAX_RGB];
  const float* map_src[VL_MAX_IMAGES];
  const double* map_table[VL_MAX_IMAGES];
  double* map_dst[VL_MAX_IMAGES];
  const double* ranges;
  const float* flow_src[VL_MAX_FLOWS];
  void* flow_dst[VL_MAX_FLOWS];
  const float* maxrad;
};

__device__ __forceinline__ unsigned vl_key(float x) {
  unsigned u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float vl_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// f(key) for every value of x[0..n), each once, in no particular order: float4 loads, four in flight per thread, where x starts on 16 bytes
template <class F>
__device__ __forceinline__ void vl_for_each_key(const float* x, long n, F f) {
  const int tid = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const long n4 = n >> 2;
    long i = tid;
    for (; i + 3 * VL_THREADS < n4; i += 4 * VL_THREADS) {
      const float4 a = x4[i], b = x4[i + VL_THREADS], c = x4[i + 2 * VL_THREADS], d = x4[i + 3 * VL_THREADS];
      f(vl_key(a.x)); f(vl_key(a.y)); f(vl_key(a.z)); f(vl_key(a.w));
      f(vl_key(b.x)); f(vl_key(b.y)); f(vl_key(b.z)); f(vl_key(b.w));
      f(vl_key(c.x)); f(vl_key(c.y)); f(vl_key(c.z)); f(vl_key(c.w));
      f(vl_key(d.x)); f(vl_key(d.y)); f(vl_key(d.z)); f(vl_key(d.w));
    }
    for (; i < n4; i += VL_THREADS) {
      const float4 a = x4[i];
      f(vl_key(a.x)); f(vl_key(a.y)); f(vl_key(a.z)); f(vl_key(a.w));
    }
    for (long e = 4 * n4 + tid; e < n; e += VL_THREADS) f(vl_key(x[e]));
  } else {
    for (long e = tid; e < n; e += VL_THREADS) f(vl_key(x[e]));
  }
}

// The radix select of one workgroup of VL_THREADS: the keys of the four order statistics rank[0..3] of x[0..n) end up in sel[0..3] (read them after
// a __syncthreads()).  hist [4][VL_BINS], wtot [16] counts of the wavefronts' bins, sel [4] the key bits found so far + [4] the rank among the
// keys that share them: LDS.
__device__ __forceinline__ void vl_select4(const float* x, long n, const unsigned (&rank)[4], unsigned* hist, unsigned* wtot, unsigned* sel) {
  const int tid = threadIdx.x, lane = dyn_lane(), wave = dyn_wave();
  const int g = tid >> 8, t = tid & 255;  // the scan: 256 threads per rank, bins 8 t .. 8 t + 7
  for (int pass = 0; pass < 3; ++pass) {
    for (int i = tid; i < 4 * VL_BINS; i += VL_THREADS) hist[i] = 0u;
    __syncthreads();
    unsigned p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u, my_prefix = 0u, my_rank = rank[g];
    if (pass > 0) {
      p0 = sel[0]; p1 = sel[1]; p2 = sel[2]; p3 = sel[3];
      my_prefix = sel[g];
      my_rank = sel[4 + g];
    }
    if (pass == 0) {
      vl_for_each_key(x, n, [&](unsigned k) { atomicAdd(&hist[k >> 21], 1u); });
    } else {
      const int hs = pass == 1 ? 21 : 10, ds = pass == 1 ? 10 : 0;
      const unsigned dm = pass == 1 ? 2047u : 1023u;
      vl_for_each_key(x, n, [&](unsigned k) {
        const unsigned h = k >> hs, d = (k >> ds) & dm;
        if (h == p0) atomicAdd(&hist[d], 1u);
        if (h == p1) atomicAdd(&hist[VL_BINS + d], 1u);
        if (h == p2) atomicAdd(&hist[2 * VL_BINS + d], 1u);
        if (h == p3) atomicAdd(&hist[3 * VL_BINS + d], 1u);
      });
    }
    __syncthreads();
    const unsigned* hg = hist + (pass == 0 ? 0 : g * VL_BINS);
    unsigned c[8], s = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      c[j] = hg[8 * t + j];
      s += c[j];
    }
    unsigned inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    unsigned excl = inc - s;
    for (int w = 4 * g; w < wave; ++w) excl += wtot[w];
    if (my_rank >= excl && my_rank - excl < s) {  // one thread of the rank's 256: its bins hold the rank
      unsigned rem = my_rank - excl;
      int j = 0;
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        if (j == e && rem >= c[e]) {
          rem -= c[e];
          j = e + 1;
        }
      }
      const unsigned bin = (unsigned)(8 * t + j);
      sel[g] = pass == 0 ? bin : ((my_prefix << (pass == 1 ? 11 : 10)) | bin);
      sel[4 + g] = rem;
    }
  }
}

// grid: K workgroups, block VL_THREADS, LDS VL_RANGES_LDS
__global__ __launch_bounds__(VL_THREADS) void k_viewlog_ranges(VlRangesArgs a) {
  unsigned* hist = reinterpret_cast<unsigned*>(dyn_smem);  // [4][VL_BINS]
  unsigned* wtot = hist + 4 * VL_BINS;                      // [16] counts of the wavefronts' bins
  unsigned* sel = wtot + 16;                                // [4] the key bits found so far, [4] the rank among the keys that share them
  const int img = blockIdx.x, tid = threadIdx.x;
  const long n = a.n;
  const float* x = a.image[img];
  if (a.magnitude[img]) {
    float* m = a.mag_out[img];
    for (long i = tid; i < n; i += VL_THREADS) {
      const float vx = x[3 * i], vy = x[3 * i + 1], vz = x[3 * i + 2];
      m[i] = sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
    }
    __syncthreads();  // the passes below read what other threads of this workgroup wrote
    x = m;
  }
  vl_select4(x, n, a.rank, hist, wtot, sel);
  __syncthreads();
  if (tid < 2) {  // numpy's _lerp on (previous, next, gamma): the difference is an fp32 subtraction, the rest double
    const float lo = vl_unkey(sel[2 * tid]), hi = vl_unkey(sel[2 * tid + 1]);
    const float d = hi - lo;
    const double w = a.weight[tid];
    double r = w >= 0.5 ? (double)hi - (double)d * (1.0 - w) : (double)lo + (double)d * w;
    if (tid == 1) r += 1e-6;  // vmax += TINY_NUMBER (utils.py:118)
    a.ranges[2 * img + tid] = r;
  }
}

// grid (tiles, F), block VL_TILE.  maxbits [F] starts as zeros (+0.0f).
__global__ __launch_bounds__(VL_TILE) void k_viewlog_flow_max(VlFlowArgs a, unsigned* maxbits) {
  const float2* f = reinterpret_cast<const float2*>(a.flow[blockIdx.y]);
  float m = 0.f;
  for (long i = (long)blockIdx.x * VL_TILE + threadIdx.x; i < a.n; i += (long)gridDim.x * VL_TILE) {
    const float2 uv = f[i];
    float u = uv.x, v = uv.y;
    if (fabsf(u) > 200.f || fabsf(v) > 200.f) u = v = 0.f;  // UNKNOWN_FLOW_THRESH (flow_utils.py:118-129)
    m = fmaxf(m, sqrtf(u * u + v * v));
  }
  m = wave_max(m);
  if (dyn_lane() == 0) atomicMax(&maxbits[blockIdx.y], __float_as_uint(m));
}

// entry k (0..54) of make_color_wheel (flow_utils.py:17-64), channel c: floor(255 i / N) of whole numbers is the integer quotient
__device__ __forceinline__ int vl_wheel(int k, int c) {
  int r, gr, b;
  if (k < 15) { r = 255; gr = 255 * k / 15; b = 0; }
  else if (k < 21) { r = 255 - 255 * (k - 15) / 6; gr = 255; b = 0; }
  else if (k < 25) { r = 0; gr = 255; b = 255 * (k - 21) / 4; }
  else if (k < 36) { r = 0; gr = 255 - 255 * (k - 25) / 11; b = 255; }
  else if (k < 49) { r = 255 * (k - 36) / 13; gr = 0; b = 255; }
  else { r = 255; gr = 0; b = 255 - 255 * (k - 49) / 6; }
  return c == 0 ? r : (c == 1 ? gr : b);
}

// grid (cdiv(n, VL_TILE), n_rgb + n_map + n_flow), block VL_TILE
__global__ __launch_bounds__(VL_TILE) void k_viewlog_panels(VlPanelArgs a) {
  const long pix = (long)blockIdx.x * VL_TILE + threadIdx.x;
  if (pix >= a.n) return;
  int j = blockIdx.y;
  if (j < a.n_rgb) {  // img_HWC2CHW, with or without torch.clamp(x, 0, 1) (train.py:657-702, :727)
    const float* src = a.rgb_src[j] + pix * 3;
    float* dst = a.rgb_dst[j] + pix;
    const bool clamp = a.rgb_clamp[j] != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float x = src[c];
      if (clamp) {
        x = x < 0.f ? 0.f : x;
        x = x > 1.f ? 1.f : x;
      }
      dst[c * a.n] = x;
    }
    return;
  }
  j -= a.n_rgb;
  if (j < a.n_map) {  // colorize_np without mask or range (utils.py:117-125) and matplotlib's Colormap.__call__ on a float array
    const double vmin = a.ranges[2 * j], vmax = a.ranges[2 * j + 1];
    double x = (double)a.map_src[j][pix];
    x = x < vmin ? vmin : x;
    x = x > vmax ? vmax : x;
    x = (x - vmin) / (vmax - vmin);
    x = x < 0.0 ? 0.0 : x;
    x = x > 1.0 ? 1.0 : x;
    int idx = (int)(x * 256.0);
    idx = idx > 255 ? 255 : (idx < 0 ? 0 : idx);
    const double* row = a.map_table[j] + idx * 3;
    double* dst = a.map_dst[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (a.map_chw) dst[c * a.n + pix] = row[c];
      else dst[pix * 3 + c] = row[c];
    }
    return;
  }
  j -= a.n_map;
  if (j >= a.n_flow) return;
  // flow_to_image and compute_color (flow_utils.py:67-153): fp32 up to maxrad, double from the divisor on
  float u = a.flow_src[j][2 * pix], v = a.flow_src[j][2 * pix + 1];
  const bool unknown = fabsf(u) > 200.f || fabsf(v) > 200.f;
  if (unknown) u = v = 0.f;
  const double div = (double)a.maxrad[j] + 2.220446049250313e-16;  // maxrad + np.finfo(float).eps
  const double ud = (double)u / div, vd = (double)v / div;
  const double rad = sqrt(ud * ud + vd * vd);
  const double ang = atan2(-vd, -ud) / 3.141592653589793;
  const double fk = (ang + 1.0) / 2.0 * 54.0 + 1.0;
  int k0 = (int)floor(fk);
  k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);
  const int k1 = k0 + 1 == 56 ? 1 : k0 + 1;
  const double fr = fk - (double)k0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double col0 = (double)vl_wheel(k0 - 1, c) / 255.0, col1 = (double)vl_wheel(k1 - 1, c) / 255.0;
    double col = (1.0 - fr) * col0 + fr * col1;
    if (rad <= 1.0) col = 1.0 - rad * (1.0 - col);
    else col = col * 0.75;
    const double level = floor(255.0 * col);
    const unsigned char byte = unknown ? (unsigned char)0 : (unsigned char)(int)level;
    if (a.flow_u8) reinterpret_cast<unsigned char*>(a.flow_dst[j])[pix * 3 + c] = byte;
    else reinterpret_cast<float*>(a.flow_dst[j])[pix * 3 + c] = (float)((double)byte / 255.0);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static bool vl_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int dyn_viewlog_ranges(int K, int H, int W, const void* image, const int32_t* magnitude, const void* mag_out, const int32_t* rank,
                                  const double* weight, double* ranges, void* stream) {
  const char* who = "dyn_viewlog_ranges";
  DYN_REQUIRE(K >= 1 && K <= VL_MAX_IMAGES, "%s: %d images in one call (1..%d)", who, K, VL_MAX_IMAGES);
  DYN_REQUIRE(H >= 1 && W >= 1 && (long)H * W * 3 < (1L << 31), "%s: H=%d W=%d is unsupported (H, W >= 1, H*W*3 < 2^31)", who, H, W);
  DYN_REQUIRE(image && magnitude && rank && weight && ranges, "%s: image, magnitude, rank, weight and ranges are required", who);
  DYN_REQUIRE(vl_aligned(ranges, 8), "%s: ranges must start on 8 bytes", who);
  VlRangesArgs a;
  a.n = (long)H * W;
  a.ranges = ranges;
  for (int q = 0; q < 4; ++q) {
    DYN_REQUIRE(rank[q] >= 0 && rank[q] < a.n, "%s: rank %d = %d is outside 0..%ld", who, q, rank[q], a.n - 1);
    a.rank[q] = (unsigned)rank[q];
  }
  for (int q = 0; q < 2; ++q) {
    DYN_REQUIRE(weight[q] >= 0.0 && weight[q] <= 1.0, "%s: weight %d = %g is outside 0..1", who, q, weight[q]);
    a.weight[q] = weight[q];
  }
  for (int k = 0; k < VL_MAX_IMAGES; ++k) {
    a.image[k] = nullptr;
    a.mag_out[k] = nullptr;
    a.magnitude[k] = 0;
    if (k >= K) continue;
    a.image[k] = static_cast<const float* const*>(image)[k];
    a.magnitude[k] = magnitude[k] ? 1 : 0;
    DYN_REQUIRE(a.image[k] && vl_aligned(a.image[k], 4), "%s: image %d is null or not on 4 bytes", who, k);
    if (a.magnitude[k]) {
      DYN_REQUIRE(mag_out, "%s: image %d is a magnitude but mag_out is null", who, k);
      a.mag_out[k] = static_cast<float* const*>(mag_out)[k];
      DYN_REQUIRE(a.mag_out[k] && vl_aligned(a.mag_out[k], 4), "%s: mag_out %d is null or not on 4 bytes", who, k);
    }
  }
  DYN_LAUNCH(DYN_K_VIEWLOG_RANGES, who, k_viewlog_ranges, dim3(K), dim3(VL_THREADS), VL_RANGES_LDS, (hipStream_t)stream, a);
  return 0;
}

extern "C" int dyn_viewlog_flow_max(int F, int H, int W, const void* flow, float* maxrad, void* stream) {
  const char* who = "dyn_viewlog_flow_max";
  DYN_REQUIRE(F >= 1 && F <= VL_MAX_FLOWS, "%s: %d flows in one call (1..%d)", who, F, VL_MAX_FLOWS);
  DYN_REQUIRE(H >= 1 && W >= 1 && (long)H * W * 3 < (1L << 31), "%s: H=%d W=%d is unsupported (H, W >= 1, H*W*3 < 2^31)", who, H, W);
  DYN_REQUIRE(flow && maxrad, "%s: flow and maxrad are required", who);
  DYN_REQUIRE(vl_aligned(maxrad, 4), "%s: maxrad must start on 4 bytes", who);
  VlFlowArgs a;
  a.n = (long)H * W;
  for (int k = 0; k < VL_MAX_FLOWS; ++k) {
    a.flow[k] = k < F ? static_cast<const float* const*>(flow)[k] : nullptr;
    DYN_REQUIRE(k >= F || (a.flow[k] && vl_aligned(a.flow[k], 8)), "%s: flow %d is null or not on 8 bytes", who, k);
  }
  hipStream_t st = (hipStream_t)stream;
  DYN_REQUIRE(hipMemsetAsync(maxrad, 0, (size_t)F * sizeof(float), st) == hipSuccess, "%s: cannot clear maxrad", who);
  int tiles = dyn_cdiv(a.n, VL_TILE * 4);
  tiles = tiles > 256 ? 256 : tiles;
  DYN_LAUNCH(DYN_K_VIEWLOG_FLOW_MAX, who, k_viewlog_flow_max, dim3(tiles, F), dim3(VL_TILE), 0, st, a, reinterpret_cast<unsigned*>(maxrad));
  return 0;
}

extern "C" int dyn_viewlog_panels(const DynViewLogPanelsParams* p, void* stream) {
  const char* who = "dyn_viewlog_panels";
  DYN_REQUIRE(p, "%s: null params", who);
  DYN_REQUIRE(p->H >= 1 && p->W >= 1 && (long)p->H * p->W * 3 < (1L << 31), "%s: H=%d W=%d is unsupported (H, W >= 1, H*W*3 < 2^31)", who, p->H,
              p->W);
  DYN_REQUIRE(p->n_rgb >= 0 && p->n_rgb <= VL_MAX_RGB, "%s: %d rgb panels (0..%d)", who, p->n_rgb, VL_MAX_RGB);
  DYN_REQUIRE(p->n_map >= 0 && p->n_map <= VL_MAX_IMAGES, "%s: %d colour-mapped panels (0..%d)", who, p->n_map, VL_MAX_IMAGES);
  DYN_REQUIRE(p->n_flow >= 0 && p->n_flow <= VL_MAX_FLOWS, "%s: %d flow panels (0..%d)", who, p->n_flow, VL_MAX_FLOWS);
  DYN_REQUIRE(p->n_rgb + p->n_map + p->n_flow >= 1, "%s: no panel asked for", who);
  DYN_REQUIRE(p->n_rgb == 0 || (p->rgb_src && p->rgb_clamp && p->rgb_dst), "%s: rgb_src, rgb_clamp and rgb_dst are required", who);
  DYN_REQUIRE(p->n_map == 0 || (p->map_src && p->map_table && p->map_dst && p->ranges), "%s: map_src, map_table, map_dst and ranges are required",
              who);
  DYN_REQUIRE(p->n_map == 0 || vl_aligned(p->ranges, 8), "%s: ranges must start on 8 bytes", who);
  DYN_REQUIRE(p->n_flow == 0 || (p->flow_src && p->flow_dst && p->maxrad), "%s: flow_src, flow_dst and maxrad are required", who);
  DYN_REQUIRE(p->n_flow == 0 || vl_aligned(p->maxrad, 4), "%s: maxrad must start on 4 bytes", who);
  VlPanelArgs a;
  a.n_rgb = p->n_rgb; a.n_map = p->n_map; a.n_flow = p->n_flow;
  a.map_chw = p->map_chw ? 1 : 0;
  a.flow_u8 = p->flow_u8 ? 1 : 0;
  a.n = (long)p->H * p->W;
  a.ranges = p->ranges;
  a.maxrad = p->maxrad;
  for (int k = 0; k < VL_MAX_RGB; ++k) {
    const bool on = k < p->n_rgb;
    a.rgb_src[k] = on ? static_cast<const float* const*>(p->rgb_src)[k] : nullptr;
    a.rgb_dst[k] = on ? static_cast<float* const*>(p->rgb_dst)[k] : nullptr;
    a.rgb_clamp[k] = on && p->rgb_clamp[k] ? 1 : 0;
    DYN_REQUIRE(!on || (a.rgb_src[k] && a.rgb_dst[k] && vl_aligned(a.rgb_src[k], 4) && vl_aligned(a.rgb_dst[k], 4)),
                "%s: rgb panel %d: a pointer is null or not on 4 bytes", who, k);
  }
  for (int k = 0; k < VL_MAX_IMAGES; ++k) {
    const bool on = k < p->n_map;
    a.map_src[k] = on ? static_cast<const float* const*>(p->map_src)[k] : nullptr;
    a.map_table[k] = on ? static_cast<const double* const*>(p->map_table)[k] : nullptr;
    a.map_dst[k] = on ? static_cast<double* const*>(p->map_dst)[k] : nullptr;
    DYN_REQUIRE(!on || (a.map_src[k] && a.map_table[k] && a.map_dst[k] && vl_aligned(a.map_src[k], 4) && vl_aligned(a.map_table[k], 8) &&
                        vl_aligned(a.map_dst[k], 8)),
                "%s: colour-mapped panel %d: a pointer is null or not aligned to its element", who, k);
  }
  for (int k = 0; k < VL_MAX_FLOWS; ++k) {
    const bool on = k < p->n_flow;
    a.flow_src[k] = on ? static_cast<const float* const*>(p->flow_src)[k] : nullptr;
    a.flow_dst[k] = on ? static_cast<void* const*>(p->flow_dst)[k] : nullptr;
    DYN_REQUIRE(!on || (a.flow_src[k] && a.flow_dst[k] && vl_aligned(a.flow_src[k], 4) && (a.flow_u8 || vl_aligned(a.flow_dst[k], 4))),
                "%s: flow panel %d: a pointer is null or not aligned to its element", who, k);
  }
  DYN_LAUNCH(DYN_K_VIEWLOG_PANELS, who, k_viewlog_panels, dim3(dyn_cdiv(a.n, VL_TILE), a.n_rgb + a.n_map + a.n_flow), dim3(VL_TILE), 0,
             (hipStream_t)stream, a);
  return 0;
}
