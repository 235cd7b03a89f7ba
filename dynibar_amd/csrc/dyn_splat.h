// Forward splatting of RGBD source frames into virtual source views (render_source_vv.py:15-66, :118-128, :312-330) and the generic
// summation splat of the third-party `splatting` package it calls.  Included from dyn_geometry.hip: the unit is built with
// -ffp-contract=off, which the bitwise contract below needs.
//
// Determinism.  A splat is a scatter-add: source pixel (x, y) lands at (x + flow_x, y + flow_y) and adds w * value to each of its four
// bilinear corners nw, ne, sw, se (corner 0..3).  Contribution id = 4 * (y * W + x) + corner.  The sum into every output pixel is
// formed SEQUENTIALLY in ascending contribution id, starting at +0.0, so that the result does not depend on the launch, the batch or
// the device: no float atomics anywhere (their arrival order changes the bits).  The inverted index is built by a stable LSD radix
// sort of the contributions' (b, target pixel) keys, generated in id order: stability leaves every destination's list in ascending id
// order with no per-list sort.  Then one resolve pass per output pixel recomputes each listed contribution from its source pixel and
// sums it in list order.
//
//   k_splat_project   (forward form only) one lane per source pixel: flow, importance = 1/z, per-batch min / max of the importance
//   k_splat_keys      one lane per source pixel: the 4 corner keys (b * H * W + target pixel, or the sentinel B * H * W when the corner
//                     is off the image), the softmax multiplier exp(w) of the forward form; clears the list bounds
//   k_splat_radix_*   ceil(bits(B * H * W) / 8) stable passes of 8 bits: tile histogram, exclusive scan (chunks, then chunk sums), scatter
//   k_splat_bounds    start / end of every destination's run in the sorted keys
//   k_splat_resolve   one lane per (output pixel, group of 8 channels): the sums, and num / (den + eps) for the normalised forms
//
// Two chains render virtual views: one frame per call (dyn_sobel_alpha, dyn_forward_splat, dyn_vv_finish) and many frames per call
// (dyn_vv_frames, below).  Their bytes are equal because each piece of arithmetic is stated once and both chains go through it:
// k_splat_project<> (the projection), sobel_alpha (the foreground alpha), splat_walk (a destination's contributions, in list order),
// vv_disk1 and vv_byte (the epilogue), and on the host splat_project_sort (clear min / max, project, keys, sort).
#pragma once

#define SPLAT_THREADS 256
#define SPLAT_ITEMS 16
#define SPLAT_TILE (SPLAT_THREADS * SPLAT_ITEMS)  // elements per radix tile
#define SPLAT_BINS 256                           // 8-bit digits
#define SPLAT_CHUNK 4096                          // histogram entries per scan block (256 threads x 16)
#define SPLAT_GROUP 8                             // output channels per resolve lane (the forward form's 4 + 2 in one walk)

// the bilinear taps of one source pixel, exactly as the package forms them (x + flow, floor, the four products)
struct SplatTap {
  bool ok;  // some corner can be inside the image
  int x0, y0;
  float ax, bx, ay, by;  // (x0 + 1 - X), (X - x0), (y0 + 1 - Y), (Y - y0)
};
__device__ __forceinline__ SplatTap splat_tap(int x, int y, float fx, float fy, int H, int W) {
  SplatTap t;
  const float X = (float)x + fx, Y = (float)y + fy;
  // range check in float BEFORE any conversion to int: NaN fails every comparison, +-inf and 1e10 (points behind the camera through
  // the 1e-8 clamp of the depth) fall outside
  t.ok = X >= -1.f && X < (float)W && Y >= -1.f && Y < (float)H;
  t.x0 = t.y0 = 0;
  t.ax = t.bx = t.ay = t.by = 0.f;
  if (t.ok) {
    const float x0 = floorf(X), y0 = floorf(Y);
    t.x0 = (int)x0;
    t.y0 = (int)y0;
    t.ax = (x0 + 1.f) - X;
    t.bx = X - x0;
    t.ay = (y0 + 1.f) - Y;
    t.by = Y - y0;
  }
  return t;
}
__device__ __forceinline__ float splat_corner_weight(const SplatTap& t, int corner) {
  switch (corner) {
    case 0: return t.ax * t.ay;  // nw
    case 1: return t.bx * t.ay;  // ne
    case 2: return t.ax * t.by;  // sw
    default: return t.bx * t.by;  // se
  }
}

// order-preserving map of a float onto unsigned (for min / max with integer atomics)
__device__ __forceinline__ unsigned splat_ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float splat_unord(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// P = depth * K_src^-1 [x y 1]^T, Q = K_dst (R P + t); pix = Q.xy / clamp(Q.z, 1e-8); flow = pix - (x, y); importance = 1 / Q.z.
// grid (<= SPLAT_PROJECT_BLOCKS, B), grid-stride over the pixels of batch entry blockIdx.y.  minmax[2b] = ord(max), minmax[2b + 1] = ord(-min),
// zeroed first; one pair of integer atomics per workgroup (same-address atomics serialise: one pair per wave cost 0.42 ms at 8 x 288 x 512).
// Batch entry b reads the depth plane and the two intrinsics of frame b / V: V = 1 gives every entry its own (dyn_forward_splat), V views
// share those of their frame (dyn_vv_frames).  RECIP: the plane holds disparities and the depth is 1 / disparity.
#define SPLAT_PROJECT_BLOCKS 32
template <bool RECIP>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_project(const float* __restrict__ depth, const float* __restrict__ kinv,
                                                                 const float* __restrict__ rot, const float* __restrict__ kdst,
                                                                 const float* __restrict__ tr, int H, int W, int V, float* __restrict__ flow,
                                                                 float* __restrict__ imp, unsigned* __restrict__ minmax) {
  const int b = blockIdx.y, f = b / V;
  const long HW = (long)H * W;
  const float* Ki = kinv + f * 9;
  const float* Rm = rot + b * 9;
  const float* Kd = kdst + f * 9;
  const float* tv = tr + b * 3;
  float hi = -INFINITY, nlo = -INFINITY;
  for (long p = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x; p < HW; p += (long)gridDim.x * SPLAT_THREADS) {
    const int y = (int)(p / W), x = (int)(p - (long)y * W);
    const float xf = (float)x, yf = (float)y, d = RECIP ? 1.f / depth[f * HW + p] : depth[f * HW + p];
    float P[3], S[3], Q[3];
    for (int i = 0; i < 3; ++i) P[i] = ((d * Ki[i * 3]) * xf + (d * Ki[i * 3 + 1]) * yf) + (d * Ki[i * 3 + 2]);
    for (int i = 0; i < 3; ++i) S[i] = ((Rm[i * 3] * P[0] + Rm[i * 3 + 1] * P[1]) + Rm[i * 3 + 2] * P[2]) + tv[i];
    for (int i = 0; i < 3; ++i) Q[i] = (Kd[i * 3] * S[0] + Kd[i * 3 + 1] * S[1]) + Kd[i * 3 + 2] * S[2];
    const float zc = Q[2] < 1e-8f ? 1e-8f : Q[2];  // torch.clamp(z, 1e-8): NaN stays NaN
    flow[(b * 2) * HW + p] = Q[0] / zc - xf;
    flow[(b * 2 + 1) * HW + p] = Q[1] / zc - yf;
    const float im = 1.f / Q[2];
    imp[b * HW + p] = im;
    hi = fmaxf(hi, im);
    nlo = fmaxf(nlo, -im);
  }
  hi = wave_max(hi);
  nlo = wave_max(nlo);
  float* red = reinterpret_cast<float*>(dyn_smem);  // [2][waves]
  constexpr int NW = SPLAT_THREADS / DYN_WAVE;
  if (dyn_lane() == 0) {
    red[dyn_wave()] = hi;
    red[NW + dyn_wave()] = nlo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NW; ++w) {
      hi = fmaxf(hi, red[w]);
      nlo = fmaxf(nlo, red[NW + w]);
    }
    atomicMax(&minmax[2 * b], splat_ord(hi));
    atomicMax(&minmax[2 * b + 1], splat_ord(nlo));
  }
}

// keys[4i + c] for the contribution ids 4i + c of source pixel i = b * HW + p.  With imp != NULL (forward form) also
// mult[i] = exp((imp - min) / (max - min + 1e-6) * 20 - 10)  (render_source_vv.py:48-53 and the package's importance_metric.exp()).
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_keys(const float* __restrict__ flow, int H, int W, unsigned sentinel,
                                                              const float* __restrict__ imp, const unsigned* __restrict__ minmax,
                                                              float* __restrict__ mult, unsigned* __restrict__ keys, int* __restrict__ start,
                                                              int* __restrict__ end) {
  const int b = blockIdx.y;
  const long HW = (long)H * W;
  const long p = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (p >= HW) return;
  const long i = b * HW + p;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const SplatTap t = splat_tap(x, y, flow[(b * 2) * HW + p], flow[(b * 2 + 1) * HW + p], H, W);
  unsigned k[4];
  for (int c = 0; c < 4; ++c) {
    const int cx = t.x0 + (c & 1), cy = t.y0 + (c >> 1);
    k[c] = (t.ok && cx >= 0 && cx < W && cy >= 0 && cy < H) ? (unsigned)(b * HW + (long)cy * W + cx) : sentinel;
  }
  uint4 kv;
  kv.x = k[0]; kv.y = k[1]; kv.z = k[2]; kv.w = k[3];
  reinterpret_cast<uint4*>(keys)[i] = kv;
  start[i] = 0;  // the target domain is the source domain: this lane clears the list bounds of pixel i
  end[i] = 0;
  if (imp) {
    const float mx = splat_unord(minmax[2 * b]), mn = -splat_unord(minmax[2 * b + 1]);
    const float w = ((imp[i] - mn) / ((mx - mn) + 1e-6f)) * 20.f - 10.f;
    mult[i] = expf(w);
  }
}

// exclusive scan of one value per thread across the 256 threads of the workgroup; s: 256 unsigned of LDS
__device__ __forceinline__ unsigned splat_block_scan(unsigned v, unsigned* s, unsigned& total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < SPLAT_THREADS; d <<= 1) {
    const unsigned o = tid >= d ? s[tid - d] : 0u;
    __syncthreads();
    s[tid] += o;
    __syncthreads();
  }
  const unsigned incl = s[tid];
  total = s[SPLAT_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// hist[d * ntiles + tile] = number of keys of the tile whose digit is d
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_radix_hist(const unsigned* __restrict__ keys, long M, int shift, int ntiles,
                                                                    unsigned* __restrict__ hist) {
  unsigned* h = reinterpret_cast<unsigned*>(dyn_smem);
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * SPLAT_TILE;
  for (int r = 0; r < SPLAT_ITEMS; ++r) {
    const long e = base + r * SPLAT_THREADS + tid;
    if (e < M) atomicAdd(&h[(keys[e] >> shift) & (SPLAT_BINS - 1)], 1u);
  }
  __syncthreads();
  hist[(long)tid * ntiles + blockIdx.x] = h[tid];
}

// in-place exclusive scan of each SPLAT_CHUNK entries of a[0, L); the chunk totals go to sums[chunk]
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_scan_chunks(unsigned* __restrict__ a, long L, unsigned* __restrict__ sums) {
  unsigned* s = reinterpret_cast<unsigned*>(dyn_smem);
  const long base = (long)blockIdx.x * SPLAT_CHUNK + (long)threadIdx.x * (SPLAT_CHUNK / SPLAT_THREADS);
  unsigned v[SPLAT_CHUNK / SPLAT_THREADS], sum = 0;
  for (int j = 0; j < SPLAT_CHUNK / SPLAT_THREADS; ++j) {
    v[j] = base + j < L ? a[base + j] : 0u;
    sum += v[j];
  }
  unsigned total;
  unsigned run = splat_block_scan(sum, s, total);
  for (int j = 0; j < SPLAT_CHUNK / SPLAT_THREADS; ++j) {
    if (base + j < L) a[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// in-place exclusive scan of the n chunk totals (one workgroup)
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_scan_top(unsigned* __restrict__ sums, int n) {
  unsigned* s = reinterpret_cast<unsigned*>(dyn_smem);
  unsigned carry = 0;
  for (int base = 0; base < n; base += SPLAT_THREADS) {
    const int i = base + threadIdx.x;
    const unsigned v = i < n ? sums[i] : 0u;
    unsigned total;
    const unsigned ex = splat_block_scan(v, s, total);
    if (i < n) sums[i] = carry + ex;
    carry += total;
  }
}

// stable scatter of one tile by the digit at `shift`: element e goes to  (digit's offset for this tile) + (number of earlier elements of
// the tile with the same digit).  The tile is walked in rounds of 256 consecutive elements; inside a round a lane's rank among its wave's
// equal digits comes from 8 ballots, the earlier waves' counts from LDS.  vals_in == NULL: the value is the element's own index
// (the contribution id of the first pass).
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_radix_scatter(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ vals_in,
                                                                       long M, int shift, int ntiles, const unsigned* __restrict__ hist,
                                                                       const unsigned* __restrict__ sums, unsigned* __restrict__ keys_out,
                                                                       unsigned* __restrict__ vals_out) {
  unsigned* base = reinterpret_cast<unsigned*>(dyn_smem);  // [256] this tile's start per digit
  unsigned* run = base + SPLAT_BINS;                       // [256] elements of each digit placed by earlier rounds
  unsigned* wcnt = run + SPLAT_BINS;                       // [4][256] this round's count per wave and digit
  const int tid = threadIdx.x, lane = dyn_lane(), wave = dyn_wave();
  {
    const long h = (long)tid * ntiles + blockIdx.x;
    base[tid] = hist[h] + sums[h / SPLAT_CHUNK];
    run[tid] = 0;
    for (int w = 0; w < SPLAT_THREADS / DYN_WAVE; ++w) wcnt[w * SPLAT_BINS + tid] = 0;
  }
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  for (int r = 0; r < SPLAT_ITEMS; ++r) {
    const long e = (long)blockIdx.x * SPLAT_TILE + r * SPLAT_THREADS + tid;
    const bool valid = e < M;
    const unsigned key = valid ? keys_in[e] : 0u;
    const unsigned val = valid ? (vals_in ? vals_in[e] : (unsigned)e) : 0u;
    const unsigned d = (key >> shift) & (SPLAT_BINS - 1);
    unsigned long long peers = __ballot(valid);
    for (int bit = 0; bit < 8; ++bit) {
      const int set = (d >> bit) & 1;
      const unsigned long long bl = __ballot(set);
      peers &= set ? bl : ~bl;
    }
    const unsigned rank = (unsigned)__builtin_popcountll(peers & lt);
    if (valid && rank == 0) wcnt[wave * SPLAT_BINS + d] = (unsigned)__builtin_popcountll(peers);
    __syncthreads();
    if (valid) {
      unsigned pos = base[d] + run[d] + rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w * SPLAT_BINS + d];
      keys_out[pos] = key;
      vals_out[pos] = val;
    }
    __syncthreads();
    unsigned add = 0;
    for (int w = 0; w < SPLAT_THREADS / DYN_WAVE; ++w) {
      add += wcnt[w * SPLAT_BINS + tid];
      wcnt[w * SPLAT_BINS + tid] = 0;
    }
    run[tid] += add;
    __syncthreads();
  }
}

// [start, end) of every destination's run of the sorted keys (destinations without contributions keep the 0, 0 of k_splat_keys)
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_bounds(const unsigned* __restrict__ keys, long M, unsigned sentinel,
                                                                int* __restrict__ start, int* __restrict__ end) {
  const long i = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (i >= M) return;
  const unsigned k = keys[i];
  if (k >= sentinel) return;
  if (i == 0 || keys[i - 1] != k) start[k] = (int)i;
  if (i == M - 1 || keys[i + 1] != k) end[k] = (int)(i + 1);
}

// what the walk of a destination's contributions reads: the head of every resolve kernel's arguments
struct SplatLists {
  int H, W;
  const float* flow;       // [B,2,H,W]
  const float* mult;       // [B,H,W] or NULL (= 1, and the frame is not multiplied)
  float eps;
  const unsigned* ids;     // contribution ids in (destination, id) order
  const int* start;
  const int* end;
};

// The contributions of destination i = b * H * W + p, in list order (ascending id): each(w, m, src, sp) with the corner's bilinear weight,
// the multiplier, and the source pixel as b * H * W + sp.  The weight is recomputed from the source pixel's flow as k_splat_keys formed it.
template <class Each>
__device__ __forceinline__ void splat_walk(const SplatLists& l, int b, long i, Each each) {
  const long HW = (long)l.H * l.W;
  const int s = l.start[i], e = l.end[i];
  for (int k = s; k < e; ++k) {
    const unsigned id = l.ids[k];
    const long src = (long)(id >> 2);
    const long sp = src - b * HW;
    const int sy = (int)(sp / l.W), sx = (int)(sp - (long)sy * l.W);
    const SplatTap t = splat_tap(sx, sy, l.flow[(b * 2) * HW + sp], l.flow[(b * 2 + 1) * HW + sp], l.H, l.W);
    each(splat_corner_weight(t, (int)(id & 3u)), l.mult ? l.mult[src] : 1.f, src, sp);
  }
}

struct SplatResolveArgs {
  SplatLists l;
  int C;                   // frame channels (forward form: channels of src)
  const float* frame;      // generic: [B,C,H,W]; forward: src [B,H,W,C] channels-last, then the importance and a ones channel
  const float* imp;        // forward form: [B,H,W]
  int normalize;
  float* out;              // generic: [B,C,H,W]; forward: feat [B,C,H,W]
  float* disp;             // forward: [B,1,H,W]
  float* mask;             // forward: [B,1,H,W] or NULL
};

// grid (ceil(HW / 256), channel groups, B).  Per listed contribution: num_c += w * (f_c * m), den += w * m  (the package's
// torch.cat([frame * m, m]) then the summation splat).
template <bool FWD>
__global__ __launch_bounds__(SPLAT_THREADS) void k_splat_resolve(SplatResolveArgs a) {
  const int b = blockIdx.z;
  const long HW = (long)a.l.H * a.l.W;
  const long p = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int cout = FWD ? a.C + 2 : a.C;
  const int c0 = blockIdx.y * SPLAT_GROUP;
  const int nc = cout - c0 < SPLAT_GROUP ? cout - c0 : SPLAT_GROUP;
  const long i = b * HW + p;
  float num[SPLAT_GROUP];
#pragma unroll
  for (int j = 0; j < SPLAT_GROUP; ++j) num[j] = 0.f;
  float den = 0.f;
  splat_walk(a.l, b, i, [&](float w, float m, long src, long sp) {
#pragma unroll
    for (int j = 0; j < SPLAT_GROUP; ++j) {
      if (j < nc) {
        const int c = c0 + j;
        float f;
        if (FWD) f = c < a.C ? a.frame[src * a.C + c] : (c == a.C ? a.imp[src] : 1.f);
        else f = a.frame[((long)b * a.C + c) * HW + sp];
        if (a.l.mult) f = f * m;
        num[j] += w * f;
      }
    }
    if (a.normalize) den += w * m;
  });
#pragma unroll
  for (int j = 0; j < SPLAT_GROUP; ++j) {
    if (j < nc) {
      const int c = c0 + j;
      const float v = a.normalize ? num[j] / (den + a.l.eps) : num[j];
      if (!FWD || c < a.C) a.out[((long)b * a.C + c) * HW + p] = v;
      else if (c == a.C) a.disp[i] = v;
      else if (a.mask) a.mask[i] = v;
    }
  }
}

// kornia.filters.spatial_gradient(mode='sobel', normalized=False) with replicate padding, alpha = exp(-beta * |grad|)  (:118-128), at
// (y, xx) of an H x W plane whose value at (row, column) is v(row, column)
template <class Tap>
__device__ __forceinline__ float sobel_alpha(int y, int xx, int H, int W, float beta, Tap v) {
  const int ym = y > 0 ? y - 1 : 0, yp = y < H - 1 ? y + 1 : H - 1;
  const int xm = xx > 0 ? xx - 1 : 0, xp = xx < W - 1 ? xx + 1 : W - 1;
  const float gx = ((v(ym, xp) - v(ym, xm)) + 2.f * (v(y, xp) - v(y, xm))) + (v(yp, xp) - v(yp, xm));
  const float gy = ((v(yp, xm) - v(ym, xm)) + 2.f * (v(yp, xx) - v(ym, xx))) + (v(yp, xp) - v(ym, xp));
  return expf(-beta * sqrtf(gx * gx + gy * gy));
}

__global__ __launch_bounds__(SPLAT_THREADS) void k_sobel_alpha(const float* __restrict__ x, long n, int H, int W, float beta,
                                                               float* __restrict__ alpha) {
  const long i = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W;
  const long b = i / HW, p = i - b * HW;
  const int y = (int)(p / W), xx = (int)(p - (long)y * W);
  const float* img = x + b * HW;
  alpha[i] = sobel_alpha(y, xx, H, W, beta, [&](int yy, int x2) { return img[(long)yy * W + x2]; });
}

// The per-view epilogue (:313-330): rgb = clip(feat[0:3] / 255, 0, 1); m = erosion(clip(feat[3], 0, 1) > 0.5, disk(1)) with out-of-image
// neighbours not eroding; out [B,H,W,3] = uint8(255 * clip(rgb * m, 0, 1)) (truncation).
// vv_disk1: the erosion at (y, x): the pixel and its in-image neighbours are all set; set(d) is the pixel d elements from this one.
template <class Set>
__device__ __forceinline__ bool vv_disk1(int y, int x, int H, int W, Set set) {
  bool m = set(0);
  if (y > 0) m = m && set(-W);
  if (y < H - 1) m = m && set(W);
  if (x > 0) m = m && set(-1);
  if (x < W - 1) m = m && set(1);
  return m;
}
__device__ __forceinline__ unsigned vv_byte(float feat, float m) {
  float v = fminf(fmaxf(feat / 255.f, 0.f), 1.f);
  v = 255.f * fminf(fmaxf(v * m, 0.f), 1.f);
  return (unsigned)(int)v;
}

__global__ __launch_bounds__(SPLAT_THREADS) void k_vv_finish(const float* __restrict__ feat, long n, int C, int H, int W,
                                                             unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W;
  const long b = i / HW, p = i - b * HW;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const float* f = feat + b * C * HW;
  const float* al = f + 3 * HW + p;
  const float mf = vv_disk1(y, x, H, W, [&](int d) { return al[d] > 0.5f; }) ? 1.f : 0.f;
  for (int c = 0; c < 3; ++c) out[i * 3 + c] = (unsigned char)vv_byte(f[c * HW + p], mf);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The virtual views of many frames in one pass (dyn_vv_frames): batch entry b = f * V + v of the splat reads frame f = b / V, so no frame is
// copied V times.  Every value comes from the bodies the per-frame chain runs (sobel_alpha, k_splat_project<>, splat_walk, vv_byte,
// vv_disk1) and the sums run in the same ascending contribution id: the bytes equal the per-frame chain's.
//
//   k_vv_source            grid (cdiv(HW, 256), F): per frame pixel the splat's source (255 r, 255 g, 255 b, alpha) as one float4,
//                          alpha = sobel_alpha of (1 / disp) / 10 at beta = 0.5, the nine taps recomputed from disp
//   k_splat_project<true>  depth = 1 / disp and the intrinsics of frame b / V
//   k_vv_resolve           grid (cdiv(HW, 256), B): splat_walk over the four channels the epilogue reads (the splatted importance and ones
//                          channels feed nothing) and the first half of the epilogue: one dword per view pixel, bytes 0..2 = vv_byte of
//                          r, g, b unmasked, byte 3 = alpha > 0.5
//   k_vv_erode             vv_disk1 of byte 3 and the masked rgb bytes: the values are in 0..1 and the mask is 0 or 1, so clip(v * m, 0, 1)
//                          is v or 0 and the byte is the resolved one or 0
// ---------------------------------------------------------------------------------------------------------------------------------
// (1 / disp) / 10 as torch forms it for a tensor on the device it runs on: a HIP tensor over a host scalar is multiplied by the fp32
// reciprocal of the scalar, a host tensor is divided
__device__ __forceinline__ float vv_tenth(float depth, int by_division) { return by_division ? depth / 10.f : depth * (1.f / 10.f); }

__global__ __launch_bounds__(SPLAT_THREADS) void k_vv_source(const float* __restrict__ img, const float* __restrict__ disp, int H, int W,
                                                             int by_division, float4* __restrict__ rgba) {
  const long HW = (long)H * W;
  const long p = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (p >= HW) return;
  const long f = blockIdx.y;
  const int y = (int)(p / W), xx = (int)(p - (long)y * W);
  const float* d = disp + f * HW;
  const float* c = img + (f * HW + p) * 3;
  float4 o;
  o.x = c[0] * 255.f;
  o.y = c[1] * 255.f;
  o.z = c[2] * 255.f;
  o.w = sobel_alpha(y, xx, H, W, 0.5f, [&](int yy, int x2) { return vv_tenth(1.f / d[(long)yy * W + x2], by_division); });
  rgba[f * HW + p] = o;
}

struct VvResolveArgs {
  SplatLists l;
  int V;
  const float4* rgba;   // [F,H,W] (r, g, b, alpha)
  unsigned* pix;        // [B,H,W]
};

__global__ __launch_bounds__(SPLAT_THREADS) void k_vv_resolve(VvResolveArgs a) {
  const int b = blockIdx.y;
  const long HW = (long)a.l.H * a.l.W;
  const long p = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (p >= HW) return;
  const long i = b * HW + p;
  const float4* frame = a.rgba + (long)(b / a.V) * HW;
  float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, den = 0.f;
  splat_walk(a.l, b, i, [&](float w, float m, long, long sp) {
    const float4 f = frame[sp];
    n0 += w * (f.x * m);
    n1 += w * (f.y * m);
    n2 += w * (f.z * m);
    n3 += w * (f.w * m);
    den += w * m;
  });
  const float d = den + a.l.eps;
  a.pix[i] = vv_byte(n0 / d, 1.f) | (vv_byte(n1 / d, 1.f) << 8) | (vv_byte(n2 / d, 1.f) << 16) | ((n3 / d > 0.5f ? 1u : 0u) << 24);
}

// n = B * H * W view pixels; view b goes to out + b * pitch
__global__ __launch_bounds__(SPLAT_THREADS) void k_vv_erode(const unsigned* __restrict__ pix, long n, int H, int W, long pitch,
                                                            unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * SPLAT_THREADS + threadIdx.x;
  if (i >= n) return;
  const long HW = (long)H * W;
  const long b = i / HW, p = i - b * HW;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const unsigned v = pix[i];
  const bool m = vv_disk1(y, x, H, W, [&](int d) { return (pix[i + d] >> 24) != 0u; });
  unsigned char* o = out + b * pitch + p * 3;
  for (int c = 0; c < 3; ++c) o[c] = m ? (unsigned char)(v >> (8 * c)) : (unsigned char)0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
static inline size_t splat_align(size_t n) { return (n + 255) & ~(size_t)255; }

struct SplatLayout {
  long N, M;          // pixels (= destinations), contributions
  int ntiles, nchunks, passes;
  size_t keys0, keys1, vals0, vals1, start, end, hist, sums, minmax, flow, imp, mult, total;
};
static bool splat_layout(int B, int H, int W, SplatLayout& L) {
  if (B <= 0 || H <= 0 || W <= 0) return false;
  L.N = (long)B * H * W;
  if (L.N > (1L << 28)) return false;  // contribution ids and positions are 32-bit: 4 N < 2^31
  L.M = 4 * L.N;
  L.ntiles = dyn_cdiv(L.M, SPLAT_TILE);
  L.nchunks = dyn_cdiv((long)SPLAT_BINS * L.ntiles, SPLAT_CHUNK);
  int bits = 0;
  while ((1L << bits) <= L.N) ++bits;  // the sentinel N must be representable
  L.passes = (bits + 7) / 8;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += splat_align(bytes); return at; };
  L.keys0 = take(L.M * 4); L.keys1 = take(L.M * 4);
  L.vals0 = take(L.M * 4); L.vals1 = take(L.M * 4);
  L.start = take(L.N * 4); L.end = take(L.N * 4);
  L.hist = take((size_t)SPLAT_BINS * L.ntiles * 4); L.sums = take((size_t)L.nchunks * 4);
  L.minmax = take((size_t)B * 2 * 4);
  L.flow = take(L.N * 2 * 4); L.imp = take(L.N * 4); L.mult = take(L.N * 4);
  L.total = o;
  return true;
}

extern "C" size_t dyn_splat_workspace_bytes(int B, int H, int W) {
  SplatLayout L;
  return splat_layout(B, H, W, L) ? L.total : 0;
}

// keys -> sorted (keys, ids) -> list bounds.  Returns the sorted ids through *ids.
static int splat_sort(const SplatLayout& L, char* ws, unsigned** ids, hipStream_t st) {
  unsigned* kin = (unsigned*)(ws + L.keys0);
  unsigned* kout = (unsigned*)(ws + L.keys1);
  unsigned* vin = nullptr;
  unsigned* vout = (unsigned*)(ws + L.vals0);
  unsigned* vspare = (unsigned*)(ws + L.vals1);
  unsigned* hist = (unsigned*)(ws + L.hist);
  unsigned* sums = (unsigned*)(ws + L.sums);
  const long nh = (long)SPLAT_BINS * L.ntiles;
  for (int pass = 0; pass < L.passes; ++pass) {
    const int shift = 8 * pass;
    DYN_LAUNCH(DYN_K_SPLAT_SORT, "k_splat_radix_hist", k_splat_radix_hist, dim3(L.ntiles), dim3(SPLAT_THREADS), SPLAT_BINS * 4, st, kin, L.M,
               shift, L.ntiles, hist);
    DYN_LAUNCH(DYN_K_SPLAT_SORT, "k_splat_scan_chunks", k_splat_scan_chunks, dim3(L.nchunks), dim3(SPLAT_THREADS), SPLAT_THREADS * 4, st,
               hist, nh, sums);
    DYN_LAUNCH(DYN_K_SPLAT_SORT, "k_splat_scan_top", k_splat_scan_top, dim3(1), dim3(SPLAT_THREADS), SPLAT_THREADS * 4, st, sums,
               L.nchunks);
    DYN_LAUNCH(DYN_K_SPLAT_SORT, "k_splat_radix_scatter", k_splat_radix_scatter, dim3(L.ntiles), dim3(SPLAT_THREADS),
               (2 + SPLAT_THREADS / DYN_WAVE) * SPLAT_BINS * 4, st, (const unsigned*)kin, (const unsigned*)vin, L.M, shift, L.ntiles,
               (const unsigned*)hist, (const unsigned*)sums, kout, vout);
    unsigned* t = kin; kin = kout; kout = t;
    if (vin == nullptr) { vin = vout; vout = vspare; }
    else { t = vin; vin = vout; vout = t; }
  }
  DYN_LAUNCH(DYN_K_SPLAT_RESOLVE, "k_splat_bounds", k_splat_bounds, dim3(dyn_cdiv(L.M, SPLAT_THREADS)), dim3(SPLAT_THREADS), 0, st,
             (const unsigned*)kin, L.M, (unsigned)L.N, (int*)(ws + L.start), (int*)(ws + L.end));
  *ids = vin;
  return 0;
}

// The refusals every entry point ends its checks with: the workspace (on 16 bytes where float4 are kept in it), then a NaN eps.  (The
// shape refusal stays with the entry: its text names the entry's own sizes, and the entry's pointer checks come between the two.)
static int splat_admit(const char* who, const void* ws, size_t given, size_t need, bool on16, bool eps_ok) {
  DYN_REQUIRE(ws && given >= need && (!on16 || ((uintptr_t)ws & 15) == 0), "%s: workspace of %zu bytes given, %zu needed%s", who, given, need,
              on16 ? ", on 16 bytes" : "");
  DYN_REQUIRE(eps_ok, "%s: eps is NaN", who);
  return 0;
}

// The front half of a forward splat: clear min / max, k_splat_project, k_splat_keys, the sort.  Returns the sorted ids through *ids.
// B batch entries of which V share a depth plane and intrinsics (k_splat_project); recip: the planes hold disparities.
static int splat_project_sort(const char* who, const SplatLayout& L, char* ws, int B, int H, int W, int V, bool recip, const float* depth,
                              const float* kinv, const float* rot, const float* kdst, const float* tr, float* flow, float* imp, float* mult,
                              unsigned** ids, hipStream_t st) {
  unsigned* minmax = (unsigned*)(ws + L.minmax);
  if (hipMemsetAsync(minmax, 0, (size_t)B * 2 * 4, st) != hipSuccess) {
    dyn_set_error("%s: hipMemsetAsync failed", who);
    return DYN_E_LAUNCH;
  }
  const int hwblocks = dyn_cdiv((long)H * W, SPLAT_THREADS);
  const int pblocks = hwblocks < SPLAT_PROJECT_BLOCKS ? hwblocks : SPLAT_PROJECT_BLOCKS;
  DYN_LAUNCH(DYN_K_SPLAT_PROJECT, "k_splat_project", (recip ? k_splat_project<true> : k_splat_project<false>), dim3(pblocks, B),
             dim3(SPLAT_THREADS), 2 * (SPLAT_THREADS / DYN_WAVE) * 4, st, depth, kinv, rot, kdst, tr, H, W, V, flow, imp, minmax);
  DYN_LAUNCH(DYN_K_SPLAT_KEYS, "k_splat_keys", k_splat_keys, dim3(hwblocks, B), dim3(SPLAT_THREADS), 0, st, (const float*)flow, H, W,
             (unsigned)L.N, (const float*)imp, (const unsigned*)minmax, mult, (unsigned*)(ws + L.keys0), (int*)(ws + L.start), (int*)(ws + L.end));
  return splat_sort(L, ws, ids, st);
}

static SplatLists splat_lists(const SplatLayout& L, const char* ws, int H, int W, const float* flow, const float* mult, float eps,
                              const unsigned* ids) {
  return SplatLists{H, W, flow, mult, eps, ids, (const int*)(ws + L.start), (const int*)(ws + L.end)};
}

extern "C" int dyn_splat(const DynSplatParams* p, void* stream) {
  DYN_REQUIRE(p, "dyn_splat: null params");
  SplatLayout L;
  DYN_REQUIRE(p->C > 0 && splat_layout(p->B, p->H, p->W, L), "dyn_splat: bad shape B=%d C=%d H=%d W=%d (B*H*W <= 2^28)", p->B, p->C, p->H,
              p->W);
  DYN_REQUIRE(p->frame && p->flow && p->out, "dyn_splat: frame, flow and out are required");
  int rc = splat_admit("dyn_splat", p->workspace, p->workspace_bytes, L.total, false, !p->normalize || p->eps == p->eps);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)p->workspace;
  const long HW = (long)p->H * p->W;
  DYN_LAUNCH(DYN_K_SPLAT_KEYS, "k_splat_keys", k_splat_keys, dim3(dyn_cdiv(HW, SPLAT_THREADS), p->B), dim3(SPLAT_THREADS), 0, st, p->flow,
             p->H, p->W, (unsigned)L.N, (const float*)nullptr, (const unsigned*)nullptr, (float*)nullptr, (unsigned*)(ws + L.keys0),
             (int*)(ws + L.start), (int*)(ws + L.end));
  unsigned* ids = nullptr;
  rc = splat_sort(L, ws, &ids, st);
  if (rc) return rc;
  SplatResolveArgs a;
  a.l = splat_lists(L, ws, p->H, p->W, p->flow, p->multiplier, p->eps, ids);
  a.C = p->C; a.frame = p->frame; a.imp = nullptr; a.normalize = p->normalize ? 1 : 0;
  a.out = p->out; a.disp = nullptr; a.mask = nullptr;
  DYN_LAUNCH(DYN_K_SPLAT_RESOLVE, "k_splat_resolve", k_splat_resolve<false>,
             dim3(dyn_cdiv(HW, SPLAT_THREADS), dyn_cdiv(p->C, SPLAT_GROUP), p->B), dim3(SPLAT_THREADS), 0, st, a);
  return 0;
}

extern "C" int dyn_forward_splat(const DynForwardSplatParams* p, void* stream) {
  DYN_REQUIRE(p, "dyn_forward_splat: null params");
  SplatLayout L;
  DYN_REQUIRE(p->C > 0 && splat_layout(p->B, p->H, p->W, L), "dyn_forward_splat: bad shape B=%d H=%d W=%d C=%d (B*H*W <= 2^28)", p->B, p->H,
              p->W, p->C);
  DYN_REQUIRE(p->src && p->depth && p->k_src_inv && p->rot && p->k_dst && p->t, "dyn_forward_splat: src, depth, k_src_inv, rot, k_dst and t are required");
  DYN_REQUIRE(p->feat && p->disp, "dyn_forward_splat: feat and disp are required");
  int rc = splat_admit("dyn_forward_splat", p->workspace, p->workspace_bytes, L.total, false, p->eps == p->eps);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)p->workspace;
  float* flow = p->flow ? p->flow : (float*)(ws + L.flow);
  float* imp = p->importance ? p->importance : (float*)(ws + L.imp);
  float* mult = p->weight_exp ? p->weight_exp : (float*)(ws + L.mult);
  unsigned* ids = nullptr;
  rc = splat_project_sort("dyn_forward_splat", L, ws, p->B, p->H, p->W, 1, false, p->depth, p->k_src_inv, p->rot, p->k_dst, p->t, flow, imp,
                          mult, &ids, st);
  if (rc) return rc;
  SplatResolveArgs a;
  a.l = splat_lists(L, ws, p->H, p->W, flow, mult, p->eps, ids);
  a.C = p->C; a.frame = p->src; a.imp = imp; a.normalize = 1;
  a.out = p->feat; a.disp = p->disp; a.mask = p->mask;
  DYN_LAUNCH(DYN_K_SPLAT_RESOLVE, "k_splat_resolve", k_splat_resolve<true>,
             dim3(dyn_cdiv((long)p->H * p->W, SPLAT_THREADS), dyn_cdiv(p->C + 2, SPLAT_GROUP), p->B), dim3(SPLAT_THREADS), 0, st, a);
  return 0;
}

extern "C" int dyn_sobel_alpha(const float* x, int B, int H, int W, float beta, float* alpha, void* stream) {
  DYN_REQUIRE(x && alpha && B > 0 && H > 0 && W > 0, "dyn_sobel_alpha: bad argument");
  const long n = (long)B * H * W;
  DYN_LAUNCH(DYN_K_SOBEL_ALPHA, "k_sobel_alpha", k_sobel_alpha, dim3(dyn_cdiv(n, SPLAT_THREADS)), dim3(SPLAT_THREADS), 0, (hipStream_t)stream, x,
             n, H, W, beta, alpha);
  return 0;
}

extern "C" int dyn_vv_finish(const float* feat, int B, int C, int H, int W, uint8_t* out, void* stream) {
  DYN_REQUIRE(feat && out && B > 0 && H > 0 && W > 0, "dyn_vv_finish: bad argument");
  DYN_REQUIRE(C >= 4, "dyn_vv_finish: feat needs at least 4 channels (rgb, alpha), got %d", C);
  const long n = (long)B * H * W;
  DYN_LAUNCH(DYN_K_VV_FINISH, "k_vv_finish", k_vv_finish, dim3(dyn_cdiv(n, SPLAT_THREADS)), dim3(SPLAT_THREADS), 0, (hipStream_t)stream, feat,
             n, C, H, W, (unsigned char*)out);
  return 0;
}

// ---- dyn_vv_frames ---------------------------------------------------------------------------------------------------------------------
// Frames go through the splat in groups: a group is as many frames as sort in the number of 8-bit passes one frame's views need (the key of
// a group of G frames has bits(G * V * H * W) bits: at 8 x 288 x 512 one frame takes 3 passes, 13 frames still 3, 16 frames 4).
#define VV_MAX_VIEWS 65535  // views per group: blockIdx.y
struct VvLayout {
  int G;            // frames per group
  SplatLayout L;    // of a full group
  size_t rgba, total;
};
static bool vv_layout(int F, int V, int H, int W, VvLayout& Y) {
  if (F <= 0 || V <= 0 || V > VV_MAX_VIEWS || H <= 0 || W <= 0) return false;
  if ((long)F * V > (1L << 28) / ((long)H * W)) return false;  // F * V * H * W <= 2^28, without overflow
  SplatLayout one;
  if (!splat_layout(V, H, W, one)) return false;
  const long per = (long)V * H * W;
  long g = ((1L << (8 * one.passes)) - 1) / per;  // the sentinel g * per stays below 2^(8 passes)
  if (g > VV_MAX_VIEWS / V) g = VV_MAX_VIEWS / V;  // a view is a row of the grid
  Y.G = (int)(g < 1 ? 1 : (g > F ? F : g));
  if (!splat_layout(Y.G * V, H, W, Y.L)) return false;
  Y.rgba = Y.L.total;
  Y.total = Y.rgba + splat_align((size_t)Y.G * H * W * sizeof(float4));
  return true;
}

extern "C" size_t dyn_vv_frames_workspace_bytes(int F, int V, int H, int W) {
  VvLayout Y;
  return vv_layout(F, V, H, W, Y) ? Y.total : 0;
}

extern "C" int dyn_vv_frames(const DynVvFramesParams* p, void* stream) {
  const char* who = "dyn_vv_frames";
  DYN_REQUIRE(p, "%s: null params", who);
  VvLayout Y;
  DYN_REQUIRE(vv_layout(p->F, p->V, p->H, p->W, Y), "%s: bad shape F=%d V=%d H=%d W=%d (sizes >= 1, V <= 65535, F*V*H*W <= 2^28)", who, p->F, p->V, p->H, p->W);
  DYN_REQUIRE(p->img && p->disp && p->k && p->k_inv && p->rot && p->t && p->out, "%s: img, disp, k, k_inv, rot, t and out are required", who);
  DYN_REQUIRE(p->out_pitch >= (int64_t)p->H * p->W * 3, "%s: out_pitch=%ld is smaller than a view of %ld bytes", who, (long)p->out_pitch,
              (long)p->H * p->W * 3);
  int rc = splat_admit(who, p->workspace, p->workspace_bytes, Y.total, true, p->eps == p->eps);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)p->workspace;
  const long HW = (long)p->H * p->W;
  const int V = p->V, hwblocks = dyn_cdiv(HW, SPLAT_THREADS);
  float4* rgba = (float4*)(ws + Y.rgba);
  for (int f0 = 0; f0 < p->F; f0 += Y.G) {
    const int G = p->F - f0 < Y.G ? p->F - f0 : Y.G, B = G * V;
    SplatLayout L;
    DYN_REQUIRE(splat_layout(B, p->H, p->W, L) && L.total <= Y.L.total, "%s: internal: the layout of %d views does not fit", who, B);
    const float* disp = p->disp + (long)f0 * HW;
    float* flow = (float*)(ws + L.flow);
    float* imp = (float*)(ws + L.imp);
    float* mult = (float*)(ws + L.mult);
    DYN_LAUNCH(DYN_K_SOBEL_ALPHA, "k_vv_source", k_vv_source, dim3(hwblocks, G), dim3(SPLAT_THREADS), 0, st, p->img + (long)f0 * HW * 3, disp, p->H,
               p->W, p->tenth_by_division ? 1 : 0, rgba);
    unsigned* ids = nullptr;
    rc = splat_project_sort(who, L, ws, B, p->H, p->W, V, true, disp, p->k_inv + (long)f0 * 9, p->rot + (long)f0 * V * 9, p->k + (long)f0 * 9,
                            p->t + (long)f0 * V * 3, flow, imp, mult, &ids, st);
    if (rc) return rc;
    VvResolveArgs a;
    a.l = splat_lists(L, ws, p->H, p->W, flow, mult, p->eps, ids);
    a.V = V; a.rgba = rgba;
    a.pix = (unsigned*)imp;  // the importance was consumed by k_splat_keys: its plane holds the resolved pixels
    DYN_LAUNCH(DYN_K_SPLAT_RESOLVE, "k_vv_resolve", k_vv_resolve, dim3(hwblocks, B), dim3(SPLAT_THREADS), 0, st, a);
    DYN_LAUNCH(DYN_K_VV_FINISH, "k_vv_erode", k_vv_erode, dim3(dyn_cdiv(L.N, SPLAT_THREADS)), dim3(SPLAT_THREADS), 0, st, (const unsigned*)a.pix,
               L.N, p->H, p->W, (long)p->out_pitch, p->out + (long)f0 * V * p->out_pitch);
  }
  return 0;
}
