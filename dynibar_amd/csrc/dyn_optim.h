// The optimizer step of the training loop (train.py:199, :467 model.optimizer.step(); ibrnet/model.py:341-364 torch.optim.Adam over six groups):
// every tensor of every group in ONE launch.
// Included from dyn_geometry.hip: -ffp-contract=off.  The update is a contract of single fp32 operations (include/dynibar_hip.h) that a numpy
// restatement reproduces bit for bit: no product may be fused into a sum here, the division and the square root are the correctly rounded
// ones (hipcc's default for HIP, -fhip-fp32-correctly-rounded-divide-sqrt), and gfx950 keeps fp32 subnormals.
//
//   k_adam_step   grid: one workgroup of 256 threads per chunk of DYN_ADAM_CHUNK = 4096 elements (a tensor of n elements has cdiv(n, 4096)
//                 chunks, the 0-d temperature one).  The kernel is a streaming pass -- 16 bytes read and 12 (16 with the fused clearing) written
//                 per element, a few tens of MB for the whole model, ~10 us of HBM time -- so what it needs is bytes in flight, not
//                 arithmetic: a full chunk is four float4 rounds per thread whose sixteen loads all come before the first store (hipcc issues
//                 the first round's four, then the other twelve while that round computes), and at 87 VGPRs five workgroups fit a CU, so the
//                 544 workgroups of the model are all resident at once (256 CUs x 5).  Larger chunks would leave CUs idle on a parameter set
//                 most of whose tensors are smaller than one chunk anyway; smaller ones only add table entries.
//                 The workgroup reads its tensor's record through wave-uniform loads; the data pointers come from that record, so the
//                 accesses are flat_load / flat_store_dwordx4.  A chunk takes the float4 path when p, g, m and v are
//                 all 16-byte aligned at its first element (4096 elements keep the alignment of the tensor's start), else single floats.
#pragma once

#define ADAM_THREADS 256
#define ADAM_ROUNDS (DYN_ADAM_CHUNK / (4 * ADAM_THREADS))
static_assert(DYN_ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a full chunk is a whole number of float4 rounds");

struct AdamScalars {
  float a, s2, c1, c2, beta2, eps;
};

__device__ __forceinline__ void adam_update(float& p, const float g, float& m, float& v, const AdamScalars& k) {
  m = m + k.c1 * (g - m);
  v = v * k.beta2 + (k.c2 * g) * g;
  const float denom = sqrtf(v) / k.s2 + k.eps;
  p = p + (k.a * m) / denom;
}

__device__ __forceinline__ void adam_update4(float4& p, const float4& g, float4& m, float4& v, const AdamScalars& k) {
  adam_update(p.x, g.x, m.x, v.x, k);
  adam_update(p.y, g.y, m.y, v.y, k);
  adam_update(p.z, g.z, m.z, v.z, k);
  adam_update(p.w, g.w, m.w, v.w, k);
}

// grid n_chunks, block ADAM_THREADS
__global__ __launch_bounds__(ADAM_THREADS) void k_adam_step(const DynAdamTensor* __restrict__ tensors, int n_tensors, const int2* __restrict__ chunks,
                                                            int n_chunks, int zero_grads) {
  const int c = blockIdx.x, tid = threadIdx.x;
  if (c >= n_chunks) return;
  const int2 ch = chunks[c];
  if (ch.x < 0 || ch.x >= n_tensors || ch.y < 0) return;
  const DynAdamTensor t = tensors[ch.x];
  const long start = (long)ch.y * DYN_ADAM_CHUNK;
  if (t.skip || start >= t.n) return;
  const long left = t.n - start;
  const int len = left < DYN_ADAM_CHUNK ? (int)left : DYN_ADAM_CHUNK;
  float* p = t.p + start;
  float* g = t.g + start;
  float* m = t.m + start;
  float* v = t.v + start;
  AdamScalars k;
  k.a = t.a; k.s2 = t.s2; k.c1 = t.c1; k.c2 = t.c2; k.beta2 = t.beta2; k.eps = t.eps;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v);
  if ((bits & 15) != 0) {
    for (int e = tid; e < len; e += ADAM_THREADS) {
      float pe = p[e], me = m[e], ve = v[e];
      const float ge = g[e];
      adam_update(pe, ge, me, ve, k);
      p[e] = pe; m[e] = me; v[e] = ve;
      if (zero_grads) g[e] = 0.f;
    }
    return;
  }
  float4* p4 = reinterpret_cast<float4*>(p);
  float4* g4 = reinterpret_cast<float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (len == DYN_ADAM_CHUNK) {  // a full chunk: the loads of all four rounds come before the first store
    float4 pp[ADAM_ROUNDS], gg[ADAM_ROUNDS], mm[ADAM_ROUNDS], vv[ADAM_ROUNDS];
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      const int i = r * ADAM_THREADS + tid;
      pp[r] = p4[i]; gg[r] = g4[i]; mm[r] = m4[i]; vv[r] = v4[i];
    }
#pragma unroll
    for (int r = 0; r < ADAM_ROUNDS; ++r) {
      const int i = r * ADAM_THREADS + tid;
      adam_update4(pp[r], gg[r], mm[r], vv[r], k);
      p4[i] = pp[r]; m4[i] = mm[r]; v4[i] = vv[r];
      if (zero_grads) g4[i] = zero;
    }
    return;
  }
  const int n4 = len >> 2;
  for (int i = tid; i < n4; i += ADAM_THREADS) {
    float4 pe = p4[i], me = m4[i], ve = v4[i];
    const float4 ge = g4[i];
    adam_update4(pe, ge, me, ve, k);
    p4[i] = pe; m4[i] = me; v4[i] = ve;
    if (zero_grads) g4[i] = zero;
  }
  for (int e = 4 * n4 + tid; e < len; e += ADAM_THREADS) {  // the last 1..3 elements of the tensor
    float pe = p[e], me = m[e], ve = v[e];
    const float ge = g[e];
    adam_update(pe, ge, me, ve, k);
    p[e] = pe; m[e] = me; v[e] = ve;
    if (zero_grads) g[e] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int dyn_adam_step(const DynAdamParams* p, void* stream) {
  const char* who = "dyn_adam_step";
  DYN_REQUIRE(p, "%s: null params", who);
  DYN_REQUIRE(p->tensors && p->chunks, "%s: tensors and chunks are required", who);
  DYN_REQUIRE(p->n_tensors >= 1 && p->n_chunks >= 1, "%s: %d tensors in %d chunks (both >= 1)", who, p->n_tensors, p->n_chunks);
  DYN_REQUIRE((reinterpret_cast<uintptr_t>(p->tensors) & 7) == 0 && (reinterpret_cast<uintptr_t>(p->chunks) & 7) == 0,
              "%s: tensors and chunks must start on 8 bytes", who);
  DYN_LAUNCH(DYN_K_ADAM_STEP, who, k_adam_step, dim3((unsigned)p->n_chunks), dim3(ADAM_THREADS), 0, (hipStream_t)stream,
             static_cast<const DynAdamTensor*>(p->tensors), p->n_tensors, reinterpret_cast<const int2*>(p->chunks), p->n_chunks, p->zero_grads ? 1 : 0);
  return 0;
}
