// Scene preparation (save_monocular_cameras.py:90-113, monocular.py:125-204, eval_nvidia.py:387-428) on the device: the three resize modes the
// reference takes from cv2, the disk erosion it takes from skimage and np.percentile of a depth map.  The contracts are restated in
// include/dynibar_hip.h; whether they agree with the real libraries is believed, not verified (neither library was available).
// Included from dyn_geometry.hip: -ffp-contract=off.  Every product and sum below is rounded on its own, as the contracts say.
//
//   k_resize_area_u8   grid (chunks, Hd, B).  A lane makes the 4 destination bytes of one 4-byte-aligned chunk of a destination row and stores
//                      them with one dword store (bytes outside the row -- the padding of a pitched store, the neighbouring row -- are never
//                      written: a partial chunk is stored bytewise).  The taps of neighbouring lanes overlap and are served by the caches:
//                      the source is read from memory once.
//   k_resize_area_f32  grid (cdiv(Wd * C, 256), Hd, B): one fp32 value per lane; the block sum, the decimation tables or, where an axis
//                      enlarges, two taps per axis with area-mode coefficients.
//   k_resize_linear_f32  grid (cdiv(Wd, 256), Hd, B): one fp32 value per lane, four taps.
//   k_resize_nearest   the chunk scheme of the area kernel over pixels of PX bytes; with `below` the output is one byte per pixel.
//   k_erode_disk_u8    grid (cdiv(W, 64), cdiv(H, 16), B): a 16 x 64 tile with its halo of r is staged in LDS (out-of-image = 1), then a row
//                      pass writes for every staged row the distance to the row's nearest zero within r (r + 1 if none), then a column
//                      pass over the disk's 2 r + 1 row chords: out = AND over dy of (distance at row y + dy > chord(dy)).  (2 r + 1) LDS
//                      reads per pass instead of one per tap of the disk.  A lane makes 4 neighbouring outputs and stores them as a dword.
//   k_percentile_pair  the radix select of k_viewlog_ranges (dyn_viewlog.h: vl_select4), one workgroup per image, then numpy's _lerp in the
//                      arithmetic numpy uses for the call: fp32 throughout for a scalar q, double for a sequence.
#pragma once

#include <float.h>

#define IG_THREADS 256
#define IG_ERODE_TH 16
#define IG_ERODE_TW 64
#define IG_MAX_RADIUS 15
#define IG_MAX_BATCH 65535

// bytes lo..hi-1 of the little-endian word to the 4-byte-aligned address p; a whole chunk is one dword store
__device__ __forceinline__ void ig_store_chunk(unsigned char* p, unsigned word, int lo, int hi) {
  if (lo == 0 && hi == 4) {
    *reinterpret_cast<unsigned*>(p) = word;
  } else {
    for (int k = lo; k < hi; ++k) p[k] = (unsigned char)(word >> (8 * k));
  }
}

__device__ __forceinline__ int ig_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct IgAreaArgs {
  const unsigned char* src;
  unsigned char* dst;
  long src_image, dst_pitch;  // bytes from one image to the next
  int Hs, Ws, Hd, Wd;
  int integer, ix, iy;        // the integer-scale branch and its block
  const int *xcount, *xidx, *ycount, *yidx;
  const float *xw, *yw;
  int Kx, Ky;
};

template <int C>
__global__ __launch_bounds__(IG_THREADS) void k_resize_area_u8(IgAreaArgs a) {
  const int y = blockIdx.y;
  const int rowbytes = a.Wd * C;
  unsigned char* row = a.dst + (long)blockIdx.z * a.dst_pitch + (long)y * rowbytes;
  const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
  const int e0 = 4 * (int)(blockIdx.x * IG_THREADS + threadIdx.x) - mis;  // the row's byte at the start of this lane's chunk
  if (e0 >= rowbytes) return;
  const unsigned char* S = a.src + (long)blockIdx.z * a.src_image;
  const int lo = e0 < 0 ? -e0 : 0, hi = rowbytes - e0 < 4 ? rowbytes - e0 : 4;
  unsigned word = 0u;
  for (int k = lo; k < hi; ++k) {
    const int e = e0 + k, dx = e / C, c = e - dx * C;
    float v;
    if (a.integer) {
      int sum = 0;
      for (int q = 0; q < a.iy; ++q) {
        const unsigned char* srow = S + ((long)ig_clamp(y * a.iy + q, a.Hs - 1) * a.Ws) * C + c;
        for (int p = 0; p < a.ix; ++p) sum += srow[(long)ig_clamp(dx * a.ix + p, a.Ws - 1) * C];
      }
      if (a.ix == 2 && a.iy == 2) v = (float)((sum + 2) >> 2);
      else v = rintf((float)sum * (1.f / (float)(a.ix * a.iy)));
    } else {
      const int ny = ig_clamp(a.ycount[y], a.Ky), nx = ig_clamp(a.xcount[dx], a.Kx);
      const int* xi = a.xidx + (long)dx * a.Kx;
      const float* xw = a.xw + (long)dx * a.Kx;
      float out = 0.f;
      for (int q = 0; q < ny; ++q) {
        const unsigned char* srow = S + ((long)ig_clamp(a.yidx[(long)y * a.Ky + q], a.Hs - 1) * a.Ws) * C + c;
        float rv = 0.f;
        for (int p = 0; p < nx; ++p) rv = rv + (float)srow[(long)ig_clamp(xi[p], a.Ws - 1) * C] * xw[p];
        const float t = a.yw[(long)y * a.Ky + q] * rv;
        out = q == 0 ? t : out + t;
      }
      v = rintf(out);  // ties to even
    }
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    word |= (unsigned)(int)v << (8 * k);
  }
  ig_store_chunk(row + e0, word, lo, hi);
}

struct IgAreaF32Args {
  const float* src;
  float* dst;
  long src_image, dst_pitch;  // bytes from one image to the next
  int Hs, Ws, Hd, Wd, C;
  int mode;                   // IG_AREA_BLOCK, IG_AREA_TABLE or IG_AREA_ENLARGE
  int ix, iy;                 // the block of the integer-scale branch (1, 1: the copy)
  const int *xcount, *xidx, *ycount, *yidx;
  const float *xw, *yw;
  int Kx, Ky;
  double scale_x, scale_y, inv_x, inv_y;  // the enlarging branch: scale = 1 / inv, inv = (double)d / s
};
#define IG_AREA_BLOCK 0
#define IG_AREA_TABLE 1
#define IG_AREA_ENLARGE 2

// the two-tap coefficient of INTER_AREA where an axis enlarges: source index and the weight of the second tap
__device__ __forceinline__ void ig_area_tap(int d, double scale, double inv, int& s, float& f) {
  s = (int)floor((double)d * scale);
  f = (float)((double)(d + 1) - (double)(s + 1) * inv);
  f = f <= 0.f ? 0.f : f - floorf(f);
}

// grid (cdiv(Wd * C, 256), Hd, B): one fp32 value per lane
__global__ __launch_bounds__(IG_THREADS) void k_resize_area_f32(IgAreaF32Args a) {
  const int e = blockIdx.x * IG_THREADS + threadIdx.x, y = blockIdx.y, C = a.C;
  if (e >= a.Wd * C) return;
  const int dx = e / C, c = e - dx * C;
  const float* S = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(a.src) + (long)blockIdx.z * a.src_image);
  float v;
  if (a.mode == IG_AREA_BLOCK) {
    const int area = a.ix * a.iy;
    if (area == 1) {
      v = S[((long)y * a.Ws + dx) * C + c];  // equal sizes: the copy
    } else {
      auto tap = [&](int k) {  // k = q * ix + p: row q, column p of the block
        const int q = k / a.ix, p = k - q * a.ix;
        return S[((long)ig_clamp(y * a.iy + q, a.Hs - 1) * a.Ws + ig_clamp(dx * a.ix + p, a.Ws - 1)) * C + c];
      };
      float sum = 0.f;
      int k = 0;
      for (; k <= area - 4; k += 4) sum = sum + (((tap(k) + tap(k + 1)) + tap(k + 2)) + tap(k + 3));
      for (; k < area; ++k) sum = sum + tap(k);
      v = sum * (1.f / (float)area);
    }
  } else if (a.mode == IG_AREA_TABLE) {
    const int ny = ig_clamp(a.ycount[y], a.Ky), nx = ig_clamp(a.xcount[dx], a.Kx);
    const int* xi = a.xidx + (long)dx * a.Kx;
    const float* xw = a.xw + (long)dx * a.Kx;
    v = 0.f;
    for (int q = 0; q < ny; ++q) {
      const float* srow = S + ((long)ig_clamp(a.yidx[(long)y * a.Ky + q], a.Hs - 1) * a.Ws) * C + c;
      float rv = 0.f;
      for (int p = 0; p < nx; ++p) rv = rv + srow[(long)ig_clamp(xi[p], a.Ws - 1) * C] * xw[p];
      const float t = a.yw[(long)y * a.Ky + q] * rv;
      v = q == 0 ? t : v + t;
    }
  } else {
    int sx, sy;
    float fx, fy;
    ig_area_tap(dx, a.scale_x, a.inv_x, sx, fx);
    ig_area_tap(y, a.scale_y, a.inv_y, sy, fy);
    const bool edge = sx >= a.Ws - 1;
    if (edge) sx = a.Ws - 1;
    const float* r0 = S + ((long)ig_clamp(sy, a.Hs - 1) * a.Ws) * C + c;
    const float* r1 = S + ((long)ig_clamp(sy + 1, a.Hs - 1) * a.Ws) * C + c;
    float v0, v1;
    if (edge) {
      v0 = r0[(long)sx * C];
      v1 = r1[(long)sx * C];
    } else {
      const float wx = 1.f - fx;
      v0 = r0[(long)sx * C] * wx + r0[(long)(sx + 1) * C] * fx;
      v1 = r1[(long)sx * C] * wx + r1[(long)(sx + 1) * C] * fx;
    }
    v = v0 * (1.f - fy) + v1 * fy;
  }
  float* row = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(a.dst) + (long)blockIdx.z * a.dst_pitch) + (long)y * a.Wd * C;
  row[e] = v;
}

struct IgLinearArgs {
  const float* src;
  float* dst;
  long src_image, dst_pitch;  // bytes
  int Hs, Ws, Hd, Wd;
  double scale_x, scale_y;
  int reciprocal;  // the taps are 1.f / S (save_monocular_cameras.py:72)
  int divide;      // the result is divided by divisor in fp32 (monocular.py:162)
  float divisor;
};

__global__ __launch_bounds__(IG_THREADS) void k_resize_linear_f32(IgLinearArgs a) {
  const int x = blockIdx.x * IG_THREADS + threadIdx.x, y = blockIdx.y;
  if (x >= a.Wd) return;
  const float* S = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(a.src) + (long)blockIdx.z * a.src_image);
  float fx = (float)(((double)x + 0.5) * a.scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx = fx - (float)sx;
  if (sx < 0) {
    sx = 0;
    fx = 0.f;
  }
  const bool edge = sx >= a.Ws - 1;
  if (edge) sx = a.Ws - 1;
  float fy = (float)(((double)y + 0.5) * a.scale_y - 0.5);
  const int sy = (int)floorf(fy);
  fy = fy - (float)sy;
  const float* r0 = S + (long)ig_clamp(sy, a.Hs - 1) * a.Ws;
  const float* r1 = S + (long)ig_clamp(sy + 1, a.Hs - 1) * a.Ws;
  float v0, v1;
  if (edge) {
    v0 = r0[sx];
    v1 = r1[sx];
    if (a.reciprocal) {
      v0 = 1.f / v0;
      v1 = 1.f / v1;
    }
  } else {
    float a0 = r0[sx], a1 = r0[sx + 1], b0 = r1[sx], b1 = r1[sx + 1];
    if (a.reciprocal) {
      a0 = 1.f / a0; a1 = 1.f / a1; b0 = 1.f / b0; b1 = 1.f / b1;
    }
    const float wx = 1.f - fx;
    v0 = a0 * wx + a1 * fx;
    v1 = b0 * wx + b1 * fx;
  }
  float v = v0 * (1.f - fy) + v1 * fy;
  if (a.divide) v = v / a.divisor;
  float* row = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(a.dst) + (long)blockIdx.z * a.dst_pitch) + (long)y * a.Wd;
  row[x] = v;
}

struct IgNearestArgs {
  const unsigned char* src;
  unsigned char* dst;
  long src_image, dst_pitch;  // bytes
  int Hs, Ws, Hd, Wd;
  double scale_x, scale_y;
  int below;  // the threshold of the BELOW form
};

// PX: bytes of a source pixel; BELOW: the destination pixel is the one byte (first source byte < below)
template <int PX, bool BELOW>
__global__ __launch_bounds__(IG_THREADS) void k_resize_nearest(IgNearestArgs a) {
  constexpr int DP = BELOW ? 1 : PX;
  const int y = blockIdx.y;
  const int rowbytes = a.Wd * DP;
  unsigned char* row = a.dst + (long)blockIdx.z * a.dst_pitch + (long)y * rowbytes;
  const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
  const int e0 = 4 * (int)(blockIdx.x * IG_THREADS + threadIdx.x) - mis;
  if (e0 >= rowbytes) return;
  int sy = (int)floor((double)y * a.scale_y);
  sy = sy > a.Hs - 1 ? a.Hs - 1 : sy;
  const unsigned char* srow = a.src + (long)blockIdx.z * a.src_image + (long)sy * a.Ws * PX;
  const int lo = e0 < 0 ? -e0 : 0, hi = rowbytes - e0 < 4 ? rowbytes - e0 : 4;
  unsigned word = 0u;
  for (int k = lo; k < hi; ++k) {
    const int e = e0 + k, dx = e / DP, c = e - dx * DP;
    int sx = (int)floor((double)dx * a.scale_x);
    sx = sx > a.Ws - 1 ? a.Ws - 1 : sx;
    const unsigned s = srow[(long)sx * PX + c];
    word |= (BELOW ? ((int)s < a.below ? 1u : 0u) : s) << (8 * k);
  }
  ig_store_chunk(row + e0, word, lo, hi);
}

struct IgErodeArgs {
  const unsigned char* src;
  unsigned char* dst;
  long src_image, dst_pitch;  // bytes
  int H, W, r;
  int chord[IG_MAX_RADIUS + 1];  // chord[|dy|] = the largest c with c*c + dy*dy <= r*r
};

__global__ __launch_bounds__(IG_THREADS) void k_erode_disk_u8(IgErodeArgs a) {
  const int r = a.r, tw = IG_ERODE_TW + 2 * r, th = IG_ERODE_TH + 2 * r, tid = threadIdx.x;
  unsigned char* tile = reinterpret_cast<unsigned char*>(dyn_smem);  // [th][tw]
  unsigned char* dist = tile + th * tw;                               // [th][IG_ERODE_TW]
  const int x0 = blockIdx.x * IG_ERODE_TW, y0 = blockIdx.y * IG_ERODE_TH;
  const unsigned char* S = a.src + (long)blockIdx.z * a.src_image;
  for (int i = tid; i < th * tw; i += IG_THREADS) {  // the tile and its halo; a tap outside the image does not count: it is staged as 1
    const int ly = i / tw, lx = i - ly * tw, gy = y0 - r + ly, gx = x0 - r + lx;
    const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    tile[i] = in ? (S[(long)gy * a.W + gx] != 0 ? 1 : 0) : 1;
  }
  __syncthreads();
  for (int i = tid; i < th * IG_ERODE_TW; i += IG_THREADS) {  // per staged row: the distance to the nearest zero of the row, r + 1 if none within r
    const int ly = i / IG_ERODE_TW, lx = i - ly * IG_ERODE_TW;
    const unsigned char* t = tile + ly * tw + lx + r;
    int d = r + 1;
    for (int dx = r; dx >= 0; --dx) {
      if (t[dx] == 0 || t[-dx] == 0) d = dx;
    }
    dist[i] = (unsigned char)d;
  }
  __syncthreads();
  const int ly = tid >> 4, lx = (tid & 15) * 4, y = y0 + ly, x = x0 + lx;
  if (y >= a.H || x >= a.W) return;
  unsigned word = 0u;
  const int n = a.W - x < 4 ? a.W - x : 4;
  for (int k = 0; k < n; ++k) {
    unsigned v = 1u;
    for (int dy = -r; dy <= r; ++dy) {
      if ((int)dist[(ly + r + dy) * IG_ERODE_TW + lx + k] <= a.chord[dy < 0 ? -dy : dy]) v = 0u;
    }
    word |= v << (8 * k);
  }
  unsigned char* p = a.dst + (long)blockIdx.z * a.dst_pitch + (long)y * a.W + x;
  if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    *reinterpret_cast<unsigned*>(p) = word;
  } else {
    for (int k = 0; k < n; ++k) p[k] = (unsigned char)(word >> (8 * k));
  }
}

struct IgPercentileArgs {
  const float* x;
  long n, stride;  // values per image, elements from one image to the next
  unsigned rank[4];
  double weight[2];
  int single;      // numpy's arithmetic for a scalar q on fp32 data: fp32 throughout
  void* out;       // [B][2]: fp32 if single, else double
};

// grid: B workgroups, block VL_THREADS, LDS VL_RANGES_LDS
__global__ __launch_bounds__(VL_THREADS) void k_percentile_pair(IgPercentileArgs a) {
  unsigned* hist = reinterpret_cast<unsigned*>(dyn_smem);
  unsigned* wtot = hist + 4 * VL_BINS;
  unsigned* sel = wtot + 16;
  vl_select4(a.x + (long)blockIdx.x * a.stride, a.n, a.rank, hist, wtot, sel);
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 2) {  // numpy's _lerp on (previous, next, gamma)
    const float lo = vl_unkey(sel[2 * tid]), hi = vl_unkey(sel[2 * tid + 1]);
    const float d = hi - lo;
    if (a.single) {
      const float w = (float)a.weight[tid];
      reinterpret_cast<float*>(a.out)[2 * (long)blockIdx.x + tid] = w >= 0.5f ? hi - d * (1.f - w) : lo + d * w;
    } else {
      const double w = a.weight[tid];
      reinterpret_cast<double*>(a.out)[2 * (long)blockIdx.x + tid] = w >= 0.5 ? (double)hi - (double)d * (1.0 - w) : (double)lo + (double)d * w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static double ig_scale(int s, int d) { return 1.0 / ((double)d / s); }
static bool ig_integer_scale(double scale) { return fabs(scale - (int)scale) < DBL_EPSILON; }

#define IG_REQUIRE_IMAGES(who, B, Hs, Ws, Hd, Wd, px)                                                                                  \
  DYN_REQUIRE((B) >= 1 && (B) <= IG_MAX_BATCH, "%s: B=%d is unsupported (1..%d)", who, (B), IG_MAX_BATCH);                             \
  DYN_REQUIRE((Hs) >= 1 && (Ws) >= 1 && (Hd) >= 1 && (Wd) >= 1 && (Hd) <= 65535 && (long)(Hs) * (Ws) * (px) < (1L << 31) &&            \
                  (long)(Hd) * (Wd) * (px) < (1L << 31),                                                                              \
              "%s: %d x %d -> %d x %d is unsupported (sizes >= 1, Hd <= 65535, H*W*bytes < 2^31)", who, (Hs), (Ws), (Hd), (Wd))

extern "C" int dyn_resize_area_u8(int B, int Hs, int Ws, int C, int Hd, int Wd, const void* src, void* dst, int64_t dst_pitch, const int32_t* xcount,
                                  const int32_t* xidx, const float* xw, int Kx, const int32_t* ycount, const int32_t* yidx, const float* yw, int Ky,
                                  void* stream) {
  const char* who = "dyn_resize_area_u8";
  DYN_REQUIRE(C == 1 || C == 3 || C == 4, "%s: C=%d is unsupported (1, 3 or 4)", who, C);
  IG_REQUIRE_IMAGES(who, B, Hs, Ws, Hd, Wd, C);
  DYN_REQUIRE(Hd <= Hs && Wd <= Ws, "%s: %d x %d -> %d x %d enlarges an axis: INTER_AREA is built for shrinking only", who, Hs, Ws, Hd, Wd);
  DYN_REQUIRE(src && dst, "%s: src and dst are required", who);
  DYN_REQUIRE(dst_pitch >= (int64_t)Hd * Wd * C, "%s: dst_pitch=%ld is smaller than an image of %ld bytes", who, (long)dst_pitch, (long)Hd * Wd * C);
  IgAreaArgs a;
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.src_image = (long)Hs * Ws * C;
  a.dst_pitch = dst_pitch;
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  const double sx = ig_scale(Ws, Wd), sy = ig_scale(Hs, Hd);
  a.integer = ig_integer_scale(sx) && ig_integer_scale(sy) ? 1 : 0;
  a.ix = (int)sx; a.iy = (int)sy;
  a.xcount = xcount; a.xidx = xidx; a.xw = xw; a.Kx = Kx;
  a.ycount = ycount; a.yidx = yidx; a.yw = yw; a.Ky = Ky;
  if (a.integer) {
    DYN_REQUIRE((long)a.ix * Wd == Ws && (long)a.iy * Hd == Hs, "%s: integer scales %d, %d do not tile %d x %d", who, a.iy, a.ix, Hs, Ws);
  } else {
    DYN_REQUIRE(xcount && xidx && xw && ycount && yidx && yw && Kx >= 1 && Ky >= 1, "%s: the decimation tables of both axes are required", who);
    DYN_REQUIRE(vl_aligned(xcount, 4) && vl_aligned(xidx, 4) && vl_aligned(xw, 4) && vl_aligned(ycount, 4) && vl_aligned(yidx, 4) && vl_aligned(yw, 4),
                "%s: the tables must start on 4 bytes", who);
  }
  const dim3 grid(dyn_cdiv((long)Wd * C + 3, 4 * IG_THREADS), Hd, B);
  hipStream_t st = (hipStream_t)stream;
  if (C == 1) DYN_LAUNCH(DYN_K_RESIZE_AREA, who, k_resize_area_u8<1>, grid, dim3(IG_THREADS), 0, st, a);
  else if (C == 3) DYN_LAUNCH(DYN_K_RESIZE_AREA, who, k_resize_area_u8<3>, grid, dim3(IG_THREADS), 0, st, a);
  else DYN_LAUNCH(DYN_K_RESIZE_AREA, who, k_resize_area_u8<4>, grid, dim3(IG_THREADS), 0, st, a);
  return 0;
}

extern "C" int dyn_resize_area_f32(int B, int Hs, int Ws, int C, int Hd, int Wd, const float* src, float* dst, int64_t dst_pitch,
                                   const int32_t* xcount, const int32_t* xidx, const float* xw, int Kx, const int32_t* ycount, const int32_t* yidx,
                                   const float* yw, int Ky, void* stream) {
  const char* who = "dyn_resize_area_f32";
  DYN_REQUIRE(C >= 1 && C <= 4, "%s: C=%d is unsupported (1..4)", who, C);
  IG_REQUIRE_IMAGES(who, B, Hs, Ws, Hd, Wd, 4 * C);
  DYN_REQUIRE(src && dst && vl_aligned(src, 4) && vl_aligned(dst, 4), "%s: src and dst are required, on 4 bytes", who);
  DYN_REQUIRE(dst_pitch >= (int64_t)Hd * Wd * C * 4 && dst_pitch % 4 == 0, "%s: dst_pitch=%ld must be a multiple of 4 and at least %ld", who,
              (long)dst_pitch, (long)Hd * Wd * C * 4);
  IgAreaF32Args a;
  a.src = src; a.dst = dst;
  a.src_image = (long)Hs * Ws * C * 4;
  a.dst_pitch = dst_pitch;
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd; a.C = C;
  a.scale_x = ig_scale(Ws, Wd); a.scale_y = ig_scale(Hs, Hd);
  a.inv_x = (double)Wd / Ws; a.inv_y = (double)Hd / Hs;
  a.ix = (int)a.scale_x; a.iy = (int)a.scale_y;
  a.xcount = xcount; a.xidx = xidx; a.xw = xw; a.Kx = Kx;
  a.ycount = ycount; a.yidx = yidx; a.yw = yw; a.Ky = Ky;
  if (Hd > Hs || Wd > Ws) {
    a.mode = IG_AREA_ENLARGE;
  } else if (ig_integer_scale(a.scale_x) && ig_integer_scale(a.scale_y)) {
    a.mode = IG_AREA_BLOCK;
    DYN_REQUIRE((long)a.ix * Wd == Ws && (long)a.iy * Hd == Hs, "%s: integer scales %d, %d do not tile %d x %d", who, a.iy, a.ix, Hs, Ws);
  } else {
    a.mode = IG_AREA_TABLE;
    DYN_REQUIRE(xcount && xidx && xw && ycount && yidx && yw && Kx >= 1 && Ky >= 1, "%s: the decimation tables of both axes are required", who);
    DYN_REQUIRE(vl_aligned(xcount, 4) && vl_aligned(xidx, 4) && vl_aligned(xw, 4) && vl_aligned(ycount, 4) && vl_aligned(yidx, 4) && vl_aligned(yw, 4),
                "%s: the tables must start on 4 bytes", who);
  }
  DYN_LAUNCH(DYN_K_RESIZE_AREA, who, k_resize_area_f32, dim3(dyn_cdiv((long)Wd * C, IG_THREADS), Hd, B), dim3(IG_THREADS), 0, (hipStream_t)stream,
             a);
  return 0;
}

extern "C" int dyn_resize_linear_f32(int B, int Hs, int Ws, int Hd, int Wd, const float* src, float* dst, int64_t dst_pitch, int reciprocal,
                                     int divide, float divisor, void* stream) {
  const char* who = "dyn_resize_linear_f32";
  IG_REQUIRE_IMAGES(who, B, Hs, Ws, Hd, Wd, 4);
  DYN_REQUIRE(src && dst && vl_aligned(src, 4) && vl_aligned(dst, 4), "%s: src and dst are required, on 4 bytes", who);
  DYN_REQUIRE(dst_pitch >= (int64_t)Hd * Wd * 4 && dst_pitch % 4 == 0, "%s: dst_pitch=%ld must be a multiple of 4 and at least %ld", who,
              (long)dst_pitch, (long)Hd * Wd * 4);
  DYN_REQUIRE(!divide || (divisor == divisor && divisor != 0.f), "%s: the divisor is zero or not a number", who);
  IgLinearArgs a;
  a.src = src; a.dst = dst;
  a.src_image = (long)Hs * Ws * 4;
  a.dst_pitch = dst_pitch;
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.scale_x = ig_scale(Ws, Wd);
  a.scale_y = ig_scale(Hs, Hd);
  a.reciprocal = reciprocal ? 1 : 0;
  a.divide = divide ? 1 : 0;
  a.divisor = divide ? divisor : 1.f;
  DYN_LAUNCH(DYN_K_RESIZE_LINEAR, who, k_resize_linear_f32, dim3(dyn_cdiv(Wd, IG_THREADS), Hd, B), dim3(IG_THREADS), 0, (hipStream_t)stream, a);
  return 0;
}

extern "C" int dyn_resize_nearest(int B, int Hs, int Ws, int pixel_bytes, int Hd, int Wd, const void* src, void* dst, int64_t dst_pitch, int below,
                                  void* stream) {
  const char* who = "dyn_resize_nearest";
  DYN_REQUIRE(pixel_bytes == 1 || pixel_bytes == 3 || pixel_bytes == 4 || pixel_bytes == 8 || pixel_bytes == 12,
              "%s: pixels of %d bytes are unsupported (1, 3, 4, 8 or 12)", who, pixel_bytes);
  IG_REQUIRE_IMAGES(who, B, Hs, Ws, Hd, Wd, pixel_bytes);
  DYN_REQUIRE(src && dst, "%s: src and dst are required", who);
  DYN_REQUIRE(below >= -1 && below <= 256, "%s: below=%d is outside 0..256 (-1: plain copy of the pixel)", who, below);
  const int dp = below >= 0 ? 1 : pixel_bytes;
  DYN_REQUIRE(dst_pitch >= (int64_t)Hd * Wd * dp, "%s: dst_pitch=%ld is smaller than an image of %ld bytes", who, (long)dst_pitch, (long)Hd * Wd * dp);
  IgNearestArgs a;
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.src_image = (long)Hs * Ws * pixel_bytes;
  a.dst_pitch = dst_pitch;
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.scale_x = ig_scale(Ws, Wd);
  a.scale_y = ig_scale(Hs, Hd);
  a.below = below;
  const dim3 grid(dyn_cdiv((long)Wd * dp + 3, 4 * IG_THREADS), Hd, B), block(IG_THREADS);
  hipStream_t st = (hipStream_t)stream;
#define IG_NEAREST(PX)                                                                                             \
  do {                                                                                                             \
    if (below >= 0) DYN_LAUNCH(DYN_K_RESIZE_NEAREST, who, (k_resize_nearest<PX, true>), grid, block, 0, st, a);   \
    else DYN_LAUNCH(DYN_K_RESIZE_NEAREST, who, (k_resize_nearest<PX, false>), grid, block, 0, st, a);             \
  } while (0)
  switch (pixel_bytes) {
    case 1: IG_NEAREST(1); break;
    case 3: IG_NEAREST(3); break;
    case 4: IG_NEAREST(4); break;
    case 8: IG_NEAREST(8); break;
    default: IG_NEAREST(12); break;
  }
#undef IG_NEAREST
  return 0;
}

extern "C" int dyn_erode_disk_u8(int B, int H, int W, int radius, const void* src, void* dst, int64_t dst_pitch, void* stream) {
  const char* who = "dyn_erode_disk_u8";
  IG_REQUIRE_IMAGES(who, B, H, W, H, W, 1);
  DYN_REQUIRE(dyn_cdiv(H, IG_ERODE_TH) <= 65535, "%s: H=%d is unsupported", who, H);
  DYN_REQUIRE(radius >= 0 && radius <= IG_MAX_RADIUS, "%s: radius=%d is outside 0..%d", who, radius, IG_MAX_RADIUS);
  DYN_REQUIRE(src && dst && src != dst, "%s: src and dst are required and must differ", who);
  DYN_REQUIRE(dst_pitch >= (int64_t)H * W, "%s: dst_pitch=%ld is smaller than an image of %ld bytes", who, (long)dst_pitch, (long)H * W);
  IgErodeArgs a;
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.src_image = (long)H * W;
  a.dst_pitch = dst_pitch;
  a.H = H; a.W = W; a.r = radius;
  for (int dy = 0; dy <= IG_MAX_RADIUS; ++dy) {
    int c = -1;  // (a row beyond the radius has no chord: every distance passes)
    if (dy <= radius) {
      c = 0;
      while ((c + 1) * (c + 1) + dy * dy <= radius * radius) ++c;
    }
    a.chord[dy] = c;
  }
  const int th = IG_ERODE_TH + 2 * radius;
  const size_t lds = (size_t)(th * (IG_ERODE_TW + 2 * radius) + th * IG_ERODE_TW + 15) / 16 * 16;  // 7.3 KB at radius 15
  DYN_LAUNCH(DYN_K_ERODE_DISK, who, k_erode_disk_u8, dim3(dyn_cdiv(W, IG_ERODE_TW), dyn_cdiv(H, IG_ERODE_TH), B), dim3(IG_THREADS), lds,
             (hipStream_t)stream, a);
  return 0;
}

extern "C" int dyn_percentile_pair(int B, int64_t n, const float* x, int64_t stride, const int32_t* rank, const double* weight, int single, void* out,
                                   void* stream) {
  const char* who = "dyn_percentile_pair";
  DYN_REQUIRE(B >= 1 && B <= IG_MAX_BATCH, "%s: B=%d is unsupported (1..%d)", who, B, IG_MAX_BATCH);
  DYN_REQUIRE(n >= 1 && n < (1L << 31), "%s: n=%ld is unsupported (1 .. 2^31 - 1)", who, (long)n);
  DYN_REQUIRE(stride >= n, "%s: stride=%ld is smaller than n=%ld", who, (long)stride, (long)n);
  DYN_REQUIRE(x && rank && weight && out, "%s: x, rank, weight and out are required", who);
  DYN_REQUIRE(vl_aligned(x, 4) && vl_aligned(out, single ? 4 : 8), "%s: x must start on 4 bytes and out on its element", who);
  IgPercentileArgs a;
  a.x = x; a.n = n; a.stride = stride;
  a.single = single ? 1 : 0;
  a.out = out;
  for (int q = 0; q < 4; ++q) {
    DYN_REQUIRE(rank[q] >= 0 && rank[q] < n, "%s: rank %d = %d is outside 0..%ld", who, q, rank[q], (long)n - 1);
    a.rank[q] = (unsigned)rank[q];
  }
  for (int q = 0; q < 2; ++q) {
    DYN_REQUIRE(weight[q] >= 0.0 && weight[q] <= 1.0, "%s: weight %d = %g is outside 0..1", who, q, weight[q]);
    a.weight[q] = weight[q];
  }
  DYN_LAUNCH(DYN_K_PERCENTILE_PAIR, who, k_percentile_pair, dim3(B), dim3(VL_THREADS), VL_RANGES_LDS, (hipStream_t)stream, a);
  return 0;
}
