// The optimizer step of the training loop (train.py:199, :467 model.optimizer.step(); ibrnet/model.py:341-364 torch.optim.Adam over six groups):
// every tensor of every group in ONE launch.
// Included from dyn_geometry.hip: -ffp-contract=off.  The update is a contract of single fp32 operations (include/dynibar_hip.h) that a numpy
// restatement reproduces bit for bit: no product may be fused into a sum here, the division and the square root are the correctly rounded
// ones (hipcc's default for HIP, -fhip-fp32-correctly-rounded-divide-sqrt), and gfx950 keeps fp32 subnormals.
//
// ONE body, adam_step_chunk<Rec, GUARDED>, over ONE chunk walk (adam_chunk) and ONE element update (adam_update<EXTENDED, GUARDED>); the four
// step kernels are its instantiations.  EXTENDED is the record type: what only DynAdamXTensor has stands under `if constexpr`, so the plain
// kernels contain no instruction of it -- not a p * 1, not a g + 0.  Registers, scratch and waves per SIMD are the compiler's
// (-Rpass-analysis=kernel-resource-usage):
//   k_adam_step           <DynAdamTensor,  false>   87 VGPRs, no scratch, 5 waves per SIMD
//   k_adam_step_guarded   <DynAdamTensor,  true>    87, 0, 5     g * coef in front of the update and a wave-uniform way out for a held step;
//                                                                coef and finite come through scalar loads
//   k_adamx_step          <DynAdamXTensor, false>  104, 0, 4     weight decay in both forms, amsgrad, maximize, step counts on the device
//   k_adamx_step_guarded  <DynAdamXTensor, true>   104, 0, 4
// The grid: one workgroup of 256 threads per chunk of DYN_ADAM_CHUNK = 4096 elements (a tensor of n elements has cdiv(n, 4096) chunks, the
// 0-d temperature one).  The kernel is a streaming pass -- 16 bytes read and 12 (16 with the fused clearing) written per element, a few tens
// of MB for the whole model, ~10 us of HBM time -- so what it needs is bytes in flight, not arithmetic: a full chunk is four float4 rounds
// per thread whose sixteen loads all come before the first store (hipcc issues the first round's four, then the other twelve while that
// round computes), and at 87 VGPRs five workgroups fit a CU, so the 544 workgroups of the model are all resident at once (256 CUs x 5).
// Larger chunks would leave CUs idle on a parameter set most of whose tensors are smaller than one chunk anyway; smaller ones only add
// table entries.  The workgroup reads its tensor's record through wave-uniform loads; the data pointers come from that record, so the
// accesses are flat_load / flat_store_dwordx4.  A chunk takes the float4 path when p, g, m and v (and vmax, where the record has one) are
// all 16-byte aligned at its first element (4096 elements keep the alignment of the tensor's start), else single floats.
// What a tensor of the extended step does not use costs a wave-uniform branch: vmax is loaded and stored only where the record has one.
// amsgrad moves 36 bytes per element instead of 28; a full chunk then has twenty float4 loads in front of its first store.
//
// The guard of the step (include/dynibar_hip.h states the contract): the global gradient norm, clipping by it and skipping a step whose
// gradients are not finite, as three plain launches in stream order -- no tickets, no atomics, nothing for the host to read.
//   k_grad_sumsq    the grid of k_adam_step.  One more streaming read of the gradients (4 bytes per element): a full aligned chunk is four
//                   float4 loads per thread, all issued before the first addition.  Element e belongs to lane (e >> 2) & 255 on every path,
//                   so the double sum of a chunk does not depend on the alignment of g.  Every chunk stores its partial, a skipped one 0.0:
//                   the buffer never needs clearing.
//   k_grad_stats    one workgroup adds the partials (a few hundred doubles) and writes sumsq, norm, coef, finite and the two counters.
//   k_grad_scale    the stand-alone clip: g = g * coef in place, nothing written when coef == 1.
//   k_adam_advance  one thread per record, after an extended step in stream order: the only writer of a tensor's step and pow.  The step
//                   kernels only read them, so no workgroup sees state another has advanced.
#pragma once

#define ADAM_THREADS 256
#define ADAM_ROUNDS (DYN_ADAM_CHUNK / (4 * ADAM_THREADS))
static_assert(DYN_ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a full chunk is a whole number of float4 rounds");

template <typename Rec> constexpr bool adam_extended = false;
template <> constexpr bool adam_extended<DynAdamXTensor> = true;

// The chunk of this workgroup: its tensor's record, its first element and its 1..DYN_ADAM_CHUNK elements.  false: nothing to do -- the
// chunk lies outside the list or the records, or its tensor is skipped.  (A flag and not a way out: k_grad_sumsq still has a 0.0 to store.)
template <typename Rec>
__device__ __forceinline__ bool adam_chunk(const Rec* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks, int n_chunks,
                                           const Rec*& t, long& start, int& len) {
  const int c = blockIdx.x;
  if (c >= n_chunks) return false;
  const int2 ch = chunks[c];
  if (ch.x < 0 || ch.x >= n_tensors || ch.y < 0) return false;
  t = tensors + ch.x;
  const long n = t->n;
  start = (long)ch.y * DYN_ADAM_CHUNK;
  if (t->skip || start >= n) return false;
  const long left = n - start;
  len = left < DYN_ADAM_CHUNK ? (int)left : DYN_ADAM_CHUNK;
  return true;
}

struct AdamScalars {
  float a, s2, c1, c2, beta2, eps;
  float wd, decay;  // these four of the extended step alone
  bool maximize, ams;
};

// The contract's update of one element, in the contract's order.  coef is read under the guard alone, vm under amsgrad alone.
template <bool EXTENDED, bool GUARDED>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float& vm, const float coef, const AdamScalars& k) {
  if constexpr (EXTENDED)
    if (k.maximize) g = -g;
  if constexpr (GUARDED) g = g * coef;
  float p1 = p;
  if constexpr (EXTENDED) {
    if (k.wd != 0.f) g = g + k.wd * p;
    p1 = p * k.decay;
  }
  m = m + k.c1 * (g - m);
  v = v * k.beta2 + (k.c2 * g) * g;
  float d = v;
  if constexpr (EXTENDED)
    if (k.ams) {
      vm = (v > vm) ? v : vm;
      d = vm;
    }
  const float denom = sqrtf(d) / k.s2 + k.eps;
  p = p1 + (k.a * m) / denom;
}

template <bool EXTENDED, bool GUARDED>
__device__ __forceinline__ void adam_update4(float4& p, const float4& g, float4& m, float4& v, float4& vm, const float coef, const AdamScalars& k) {
  adam_update<EXTENDED, GUARDED>(p.x, g.x, m.x, v.x, vm.x, coef, k);
  adam_update<EXTENDED, GUARDED>(p.y, g.y, m.y, v.y, vm.y, coef, k);
  adam_update<EXTENDED, GUARDED>(p.z, g.z, m.z, v.z, vm.z, coef, k);
  adam_update<EXTENDED, GUARDED>(p.w, g.w, m.w, v.w, vm.w, coef, k);
}

// One chunk of the step, over either record.  stats is read under the guard alone.
template <typename Rec, bool GUARDED>
__device__ __forceinline__ void adam_step_chunk(const Rec* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks, int n_chunks,
                                                int zero_grads, const DynGradStats* __restrict__ stats, int skip_nonfinite) {
  constexpr bool X = adam_extended<Rec>;
  const int tid = threadIdx.x;
  const Rec* t;
  long start;
  int len;
  if (!adam_chunk(tensors, n_tensors, chunks, n_chunks, t, start, len)) return;
  float* p = t->p + start;
  float* g = t->g + start;
  float* m = t->m + start;
  float* v = t->v + start;
  float coef = 1.f;
  if constexpr (GUARDED) {
    coef = stats->coef;
    if (skip_nonfinite && stats->finite == 0) {  // a held step: p, m, v and vmax stay as they are (k_adam_advance holds step and pow)
      if (zero_grads)
        for (int e = tid; e < len; e += ADAM_THREADS) g[e] = 0.f;
      return;
    }
  }
  AdamScalars k;
  k.a = t->a; k.s2 = t->s2; k.c1 = t->c1; k.c2 = t->c2; k.beta2 = t->beta2; k.eps = t->eps;
  k.ams = false;
  float* x = v;  // vmax; without amsgrad it is never read or written, and v leaves the alignment test what it is
  if constexpr (X) {
    k.wd = t->wd; k.decay = t->decay;
    k.maximize = (t->flags & 1) != 0;
    k.ams = t->vmax != nullptr;
    if (k.ams) x = t->vmax + start;
    if (const double* pw = t->pow) {  // the tensor's own step count lives on the device: the scalars of step t + 1 from beta^t, in double
      const double b1 = pw[0] * t->beta1_d;
      const double b2 = pw[1] * t->beta2_d;
      k.a = (float)(-t->lr_d / (1.0 - b1));
      k.s2 = (float)sqrt(1.0 - b2);
    }
  }
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
                         reinterpret_cast<uintptr_t>(x);
  const bool aligned = (bits & 15) == 0;
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  float4* x4 = reinterpret_cast<float4*>(x);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (aligned && len == DYN_ADAM_CHUNK) {  // a full chunk: the loads of all four rounds come before the first store
    float4 pp[ADAM_ROUNDS], gg[ADAM_ROUNDS], mm[ADAM_ROUNDS], vv[ADAM_ROUNDS], xx[ADAM_ROUNDS];
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      const int i = r * ADAM_THREADS + tid;
      pp[r] = p4[i]; gg[r] = g4[i]; mm[r] = m4[i]; vv[r] = v4[i];
      xx[r] = zero;
      if (k.ams) xx[r] = x4[i];
    }
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      const int i = r * ADAM_THREADS + tid;
      adam_update4<X, GUARDED>(pp[r], gg[r], mm[r], vv[r], xx[r], coef, k);
      p4[i] = pp[r]; m4[i] = mm[r]; v4[i] = vv[r];
      if (k.ams) x4[i] = xx[r];
      if (zero_grads) g4[i] = zero;
    }
    return;
  }
  const int n4 = aligned ? len >> 2 : 0;
  for (int i = tid; i < n4; i += ADAM_THREADS) {
    float4 pe = p4[i], me = m4[i], ve = v4[i], xe = zero;
    if (k.ams) xe = x4[i];
    adam_update4<X, GUARDED>(pe, g4[i], me, ve, xe, coef, k);
    p4[i] = pe; m4[i] = me; v4[i] = ve;
    if (k.ams) x4[i] = xe;
    if (zero_grads) g4[i] = zero;
  }
  for (int e = 4 * n4 + tid; e < len; e += ADAM_THREADS) {  // single floats: the last 1..3 elements of the tensor, or all of an unaligned chunk
    float pe = p[e], me = m[e], ve = v[e], xe = 0.f;
    if (k.ams) xe = x[e];
    adam_update<X, GUARDED>(pe, g[e], me, ve, xe, coef, k);
    p[e] = pe; m[e] = me; v[e] = ve;
    if (k.ams) x[e] = xe;
    if (zero_grads) g[e] = 0.f;
  }
}

// the four step kernels: grid n_chunks, block ADAM_THREADS
__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step(const DynAdamTensor* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks,
                                                            int n_chunks, int zero_grads) {
  adam_step_chunk<DynAdamTensor, false>(tensors, n_tensors, chunks, n_chunks, zero_grads, nullptr, 0);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step_guarded(const DynAdamTensor* __restrict__ tensors, int n_tensors,
                                                                    const int2* __restrict__ chunks, int n_chunks, int zero_grads,
                                                                    const DynGradStats* __restrict__ stats, int skip_nonfinite) {
  adam_step_chunk<DynAdamTensor, true>(tensors, n_tensors, chunks, n_chunks, zero_grads, stats, skip_nonfinite);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adamx_step(const DynAdamXTensor* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks,
                                                             int n_chunks, int zero_grads) {
  adam_step_chunk<DynAdamXTensor, false>(tensors, n_tensors, chunks, n_chunks, zero_grads, nullptr, 0);
}

__global__ __launch_bounds__(ADAM_THREADS) void k_adamx_step_guarded(const DynAdamXTensor* __restrict__ tensors, int n_tensors,
                                                                     const int2* __restrict__ chunks, int n_chunks, int zero_grads,
                                                                     const DynGradStats* __restrict__ stats, int skip_nonfinite) {
  adam_step_chunk<DynAdamXTensor, true>(tensors, n_tensors, chunks, n_chunks, zero_grads, stats, skip_nonfinite);
}

// grid cdiv(n_tensors, ADAM_THREADS), block ADAM_THREADS.  stats may be null (the unguarded step: nothing is ever held).
__global__ __launch_bounds__(ADAM_THREADS) void k_adam_advance(const DynAdamXTensor* __restrict__ tensors, int n_tensors,
                                                               const DynGradStats* __restrict__ stats, int skip_nonfinite) {
  const int i = blockIdx.x * ADAM_THREADS + threadIdx.x;
  if (i >= n_tensors) return;
  if (stats != nullptr && skip_nonfinite && stats->finite == 0) return;
  const DynAdamXTensor* t = tensors + i;
  double* pw = t->pow;
  float* step = t->step;
  if (t->skip || pw == nullptr || step == nullptr) return;
  const double b1 = pw[0] * t->beta1_d;
  const double b2 = pw[1] * t->beta2_d;
  *step = *step + 1.0f;
  pw[0] = b1;
  pw[1] = b2;
}

// The 256 lane sums of a workgroup -> one double, the same in every thread: the xor butterfly within each wave (met_wave_sum), then
// ((w0 + w1) + w2) + w3.  Every thread of the workgroup must call it.
__device__ __forceinline__ double grad_block_sum(double v, double* red) {
  v = met_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ void grad_add(double& s, const float g) { s += (double)g * (double)g; }

#define GRAD_LDS (sizeof(double) * (ADAM_THREADS / 64))

// grid n_chunks, block ADAM_THREADS, LDS GRAD_LDS
__global__ __launch_bounds__(ADAM_THREADS) void k_grad_sumsq(const DynAdamTensor* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks,
                                                             int n_chunks, double* __restrict__ partials) {
  double* red = reinterpret_cast<double*>(dyn_smem);  // [ADAM_THREADS / 64] wave sums
  const int c = blockIdx.x, tid = threadIdx.x;
  if (c >= n_chunks) return;  // (partials has n_chunks entries)
  const DynAdamTensor* t;
  long start;
  int len;
  double s = 0.0;  // stays 0.0 for a chunk that is skipped or lies outside the records
  if (adam_chunk(tensors, n_tensors, chunks, n_chunks, t, start, len)) {
    const float* g = t->g + start;
    const int n4 = len >> 2;  // whole groups of four elements; group i belongs to lane i & 255
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
      const float4* g4 = reinterpret_cast<const float4*>(g);
      if (len == DYN_ADAM_CHUNK) {  // a full chunk: all four loads before the first addition
        float4 gg[ADAM_ROUNDS];
#pragma unroll
        for (int r = 0; r < ADAM_ROUNDS; ++r) gg[r] = g4[r * ADAM_THREADS + tid];
#pragma unroll
        for (int r = 0; r < ADAM_ROUNDS; ++r) {
          grad_add(s, gg[r].x); grad_add(s, gg[r].y); grad_add(s, gg[r].z); grad_add(s, gg[r].w);
        }
      } else {
        for (int i = tid; i < n4; i += ADAM_THREADS) {
          const float4 ge = g4[i];
          grad_add(s, ge.x); grad_add(s, ge.y); grad_add(s, ge.z); grad_add(s, ge.w);
        }
      }
    } else {
      for (int i = tid; i < n4; i += ADAM_THREADS) {
        const float* ge = g + 4 * i;
        grad_add(s, ge[0]); grad_add(s, ge[1]); grad_add(s, ge[2]); grad_add(s, ge[3]);
      }
    }
    if (tid == (n4 & (ADAM_THREADS - 1)))  // the last 1..3 elements of the tensor are group n4: after every earlier group of its lane
      for (int e = 4 * n4; e < len; ++e) grad_add(s, g[e]);
  }
  s = grad_block_sum(s, red);
  if (tid == 0) partials[c] = s;
}

// grid 1, block ADAM_THREADS, LDS GRAD_LDS
__global__ __launch_bounds__(ADAM_THREADS) void k_grad_stats(const double* __restrict__ partials, int n_chunks, DynGradStats* __restrict__ stats,
                                                             float max_norm, int count) {
  double* red = reinterpret_cast<double*>(dyn_smem);  // [ADAM_THREADS / 64] wave sums
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < n_chunks; i += ADAM_THREADS) s += partials[i];
  s = grad_block_sum(s, red);
  if (tid != 0) return;
  const int finite = __builtin_isfinite(s) ? 1 : 0;
  const float norm = (float)sqrt(s);
  float coef = 1.0f;
  if (max_norm > 0.f && finite) coef = fminf(1.0f, max_norm / (norm + 1e-6f));
  stats->sumsq = s;
  stats->norm = norm;
  stats->coef = coef;
  stats->finite = finite;
  stats->reserved = 0;
  if (count) {
    stats->calls = stats->calls + 1;
    if (!finite) stats->nonfinite = stats->nonfinite + 1;
  }
}

// grid n_chunks, block ADAM_THREADS
__global__ __launch_bounds__(ADAM_THREADS) void k_grad_scale(const DynAdamTensor* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks,
                                                             int n_chunks, const DynGradStats* __restrict__ stats) {
  const int tid = threadIdx.x;
  const float coef = stats->coef;
  if (coef == 1.0f) return;  // g * 1 is g: nothing to write
  const DynAdamTensor* t;
  long start;
  int len;
  if (!adam_chunk(tensors, n_tensors, chunks, n_chunks, t, start, len)) return;
  float* g = t->g + start;
  const int n4 = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? len >> 2 : 0;
  float4* g4 = reinterpret_cast<float4*>(g);
  for (int i = tid; i < n4; i += ADAM_THREADS) {
    const float4 ge = g4[i];
    g4[i] = make_float4(ge.x * coef, ge.y * coef, ge.z * coef, ge.w * coef);
  }
  for (int e = 4 * n4 + tid; e < len; e += ADAM_THREADS) g[e] = g[e] * coef;  // the last 1..3 elements, or all of an unaligned chunk
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
// what every entry point here refuses about the records and the chunk list
static int adam_tables_ok(const char* who, const void* tensors, int n_tensors, const void* chunks, int n_chunks) {
  DYN_REQUIRE(tensors && chunks, "%s: tensors and chunks are required", who);
  DYN_REQUIRE(n_tensors >= 1 && n_chunks >= 1, "%s: %d tensors in %d chunks (both >= 1)", who, n_tensors, n_chunks);
  DYN_REQUIRE((reinterpret_cast<uintptr_t>(tensors) & 7) == 0 && (reinterpret_cast<uintptr_t>(chunks) & 7) == 0,
              "%s: tensors and chunks must start on 8 bytes", who);
  return 0;
}

// ... and about the DynGradStats that a guarded step or the scale reads
static int adam_stats_ok(const char* who, const DynGradStats* stats) {
  DYN_REQUIRE(stats, "%s: stats is required", who);
  DYN_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "%s: stats must start on 8 bytes", who);
  return 0;
}

// The four step entry points: the checks, the step kernel of (record, guarded) and, where the caller asks, k_adam_advance behind it in
// stream order.  The unguarded ones pass no stats: nothing is ever held.
static int adam_step(const char* who, bool extended, bool guarded, const void* tensors, int n_tensors, const int32_t* chunk_list, int n_chunks,
                     int zero_grads, const DynGradStats* stats, int skip_nonfinite, int advance, hipStream_t stream) {
  if (const int rc = adam_tables_ok(who, tensors, n_tensors, chunk_list, n_chunks)) return rc;
  if (guarded)
    if (const int rc = adam_stats_ok(who, stats)) return rc;
  const dim3 grid((unsigned)n_chunks), block(ADAM_THREADS);
  const int2* chunks = reinterpret_cast<const int2*>(chunk_list);
  const int zero = zero_grads ? 1 : 0, skip = skip_nonfinite ? 1 : 0;
  if (!extended) {
    const DynAdamTensor* recs = static_cast<const DynAdamTensor*>(tensors);
    if (guarded) DYN_LAUNCH(DYN_K_ADAM_STEP_GUARDED, who, k_adam_step_guarded, grid, block, 0, stream, recs, n_tensors, chunks, n_chunks, zero, stats, skip);
    else DYN_LAUNCH(DYN_K_ADAM_STEP, who, k_adam_step, grid, block, 0, stream, recs, n_tensors, chunks, n_chunks, zero);
    return 0;
  }
  const DynAdamXTensor* recs = static_cast<const DynAdamXTensor*>(tensors);
  if (guarded) DYN_LAUNCH(DYN_K_ADAMX_STEP_GUARDED, who, k_adamx_step_guarded, grid, block, 0, stream, recs, n_tensors, chunks, n_chunks, zero, stats, skip);
  else DYN_LAUNCH(DYN_K_ADAMX_STEP, who, k_adamx_step, grid, block, 0, stream, recs, n_tensors, chunks, n_chunks, zero);
  if (advance)
    DYN_LAUNCH(DYN_K_ADAM_ADVANCE, who, k_adam_advance, dim3((unsigned)((n_tensors + ADAM_THREADS - 1) / ADAM_THREADS)), block, 0, stream, recs, n_tensors,
               stats, skip);
  return 0;
}

extern "C" int dyn_adam_step(const DynAdamParams* p, void* stream) {
  const char* who = "dyn_adam_step";
  DYN_REQUIRE(p, "%s: null params", who);
  return adam_step(who, false, false, p->tensors, p->n_tensors, p->chunks, p->n_chunks, p->zero_grads, nullptr, 0, 0, (hipStream_t)stream);
}

extern "C" int dyn_adam_step_guarded(const DynAdamGuardedParams* p, void* stream) {
  const char* who = "dyn_adam_step_guarded";
  DYN_REQUIRE(p, "%s: null params", who);
  return adam_step(who, false, true, p->tensors, p->n_tensors, p->chunks, p->n_chunks, p->zero_grads, p->stats, p->skip_nonfinite, 0, (hipStream_t)stream);
}

extern "C" int dyn_adamx_step(const DynAdamXParams* p, void* stream) {
  const char* who = "dyn_adamx_step";
  DYN_REQUIRE(p, "%s: null params", who);
  return adam_step(who, true, false, p->tensors, p->n_tensors, p->chunks, p->n_chunks, p->zero_grads, nullptr, 0, p->advance, (hipStream_t)stream);
}

extern "C" int dyn_adamx_step_guarded(const DynAdamXGuardedParams* p, void* stream) {
  const char* who = "dyn_adamx_step_guarded";
  DYN_REQUIRE(p, "%s: null params", who);
  return adam_step(who, true, true, p->tensors, p->n_tensors, p->chunks, p->n_chunks, p->zero_grads, p->stats, p->skip_nonfinite, p->advance,
                   (hipStream_t)stream);
}

extern "C" int dyn_grad_norm(const DynGradNormParams* p, void* stream) {
  const char* who = "dyn_grad_norm";
  DYN_REQUIRE(p, "%s: null params", who);
  if (const int rc = adam_tables_ok(who, p->tensors, p->n_tensors, p->chunks, p->n_chunks)) return rc;
  DYN_REQUIRE(p->partials && p->stats, "%s: partials and stats are required", who);
  DYN_REQUIRE((reinterpret_cast<uintptr_t>(p->partials) & 7) == 0 && (reinterpret_cast<uintptr_t>(p->stats) & 7) == 0,
              "%s: partials and stats must start on 8 bytes", who);
  DYN_REQUIRE(p->max_norm == p->max_norm, "%s: max_norm is NaN", who);
  DYN_LAUNCH(DYN_K_GRAD_SUMSQ, who, k_grad_sumsq, dim3((unsigned)p->n_chunks), dim3(ADAM_THREADS), GRAD_LDS, (hipStream_t)stream,
             static_cast<const DynAdamTensor*>(p->tensors), p->n_tensors, reinterpret_cast<const int2*>(p->chunks), p->n_chunks, p->partials);
  DYN_LAUNCH(DYN_K_GRAD_STATS, who, k_grad_stats, dim3(1), dim3(ADAM_THREADS), GRAD_LDS, (hipStream_t)stream,
             static_cast<const double*>(p->partials), p->n_chunks, p->stats, p->max_norm, p->count ? 1 : 0);
  return 0;
}

extern "C" int dyn_grad_scale(const DynGradScaleParams* p, void* stream) {
  const char* who = "dyn_grad_scale";
  DYN_REQUIRE(p, "%s: null params", who);
  if (const int rc = adam_tables_ok(who, p->tensors, p->n_tensors, p->chunks, p->n_chunks)) return rc;
  if (const int rc = adam_stats_ok(who, p->stats)) return rc;
  DYN_LAUNCH(DYN_K_GRAD_SCALE, who, k_grad_scale, dim3((unsigned)p->n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream,
             static_cast<const DynAdamTensor*>(p->tensors), p->n_tensors, reinterpret_cast<const int2*>(p->chunks), p->n_chunks, p->stats);
  return 0;
}
