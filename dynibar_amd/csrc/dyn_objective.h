// The training objective of the monocular main loop (train.py:300-456) and eff_distloss_native: forward, fixed-order reduction, backward.
// Included at the end of dyn_train.hip (one translation unit: the emulator build compiles the .hip units and every header they include).
//
// Layout of the work
//   k_objective_rays      one wavefront per ray, four rays per workgroup: everything whose natural unit is a ray.  The sums over the
//                         samples (weights_dy, weights_st, occ_weights) and the two prefix scans of the distortion loss walk the ray in
//                         chunks of 64 samples with a carry; lane 0 then forms the ray's scalar terms.
//   k_objective_samples   one thread per (ray, sample): consistency |pts_traj_ref - pts_traj_anchor| occ_weights and the three sf_seq terms;
//                         every tensor is read once (the neighbour along S comes from the cache line the next lane fetched).
//   k_objective_finish    one workgroup, a wavefront per column of partials: lane l adds the rows l, l + 64, ... in ascending order, the 64 lane
//                         sums are combined by a fixed butterfly -- the same order in every call, so the result is bitwise reproducible.  It forms the logged scalars
//                         and the coefficients (weight / denominator of every term) the backward multiplies with.
//   k_objective_rays_bwd / k_objective_samples_bwd   element-wise given those coefficients; neighbour terms are gathered, never scattered.
//
// Arithmetic is double wherever a sum or a cancellation is involved (the per-ray ratio and its logarithms, the prefix sums of the
// distortion loss, all partial sums): the fp32 form of the distortion gradient m_k (P_k - S_k) - (Q_k - T_k) loses digits exactly like
// the fp32 torch form does, and a product kernel should not sit on the same error as the yardstick it is compared with.  In double
// the suffix sums are taken as total - prefix (the cancellation is 1e-16 of the total), so one pair of scans serves both directions.
// The traffic (about 45 MB at 3072 x 64) and the launch count are what cost time here, not the fp64 rate.
#pragma once

#define OBJ_THREADS 256
#define OBJ_RAYS_PER_WG 4
enum {  // per-workgroup partial sums of k_objective_rays
  OBJ_N_REF, OBJ_D_REF, OBJ_N_ANC, OBJ_D_ANC, OBJ_N_DYN, OBJ_D_DYN, OBJ_N_REFDY, OBJ_D_REFDY, OBJ_N_ANCDY, OBJ_D_ANCDY, OBJ_N_DISP, OBJ_N_FLOW,
  OBJ_D_FLOW, OBJ_ENT, OBJ_DIST, OBJ_N_ST, OBJ_D_ST, OBJ_N_ST2, OBJ_D_ST2, OBJ_D_OCC, OBJ_NRAY
};
enum { OBJ_N_CYC, OBJ_SF_ABS, OBJ_SF_T2, OBJ_SF_SP, OBJ_NSMP };  // ... of k_objective_samples
enum {  // weight / denominator of every term, left in the workspace for the backward
  OBJ_C_REF, OBJ_C_ANC, OBJ_C_DYN, OBJ_C_REFDY, OBJ_C_ANCDY, OBJ_C_DISP, OBJ_C_FLOW, OBJ_C_CYC, OBJ_C_SFABS, OBJ_C_SFT, OBJ_C_SFSP, OBJ_C_ENT,
  OBJ_C_DIST, OBJ_C_ST, OBJ_C_ST2, OBJ_NCOEF
};
#define OBJ_EPS2 1e-6  /* criterion.py:19 EPSILON ** 2 */

__device__ __forceinline__ double obj_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double obj_scan_sum(double v, int lane) {  // inclusive prefix sum over the wavefront
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
__device__ __forceinline__ double obj_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }  // torch.sign: sign(0) = 0
__device__ __forceinline__ double obj_charb(double x, double t) { return sqrt((x - t) * (x - t) + OBJ_EPS2); }
__device__ __forceinline__ double obj_dcharb(double x, double t) { return (x - t) / sqrt((x - t) * (x - t) + OBJ_EPS2); }

// workspace: [coef OBJ_NCOEF][ray sums R x 2][ray partials nbr x OBJ_NRAY][sample partials nbs x OBJ_NSMP], all double
struct ObjLayout {
  long nbr, nbs;
  size_t off_rays, off_pray, off_psmp, bytes;
};
static inline ObjLayout obj_layout(long R, long S) {
  ObjLayout L;
  L.nbr = (R + OBJ_RAYS_PER_WG - 1) / OBJ_RAYS_PER_WG;
  L.nbs = (R * S + OBJ_THREADS - 1) / OBJ_THREADS;
  L.off_rays = OBJ_NCOEF * sizeof(double);
  L.off_pray = L.off_rays + (size_t)R * 2 * sizeof(double);
  L.off_psmp = L.off_pray + (size_t)L.nbr * OBJ_NRAY * sizeof(double);
  L.bytes = L.off_psmp + (size_t)L.nbs * OBJ_NSMP * sizeof(double);
  return L;
}

// ---- the distortion loss of one ray, shared by the objective and eff_distloss_native -----------------------------------------------------
// n elements; w_at(i), m_at(i), d_at(i): weight, interval midpoint and interval length of element i.  Returns (on every lane)
// (1/3) sum d w^2 + 2 sum_{i>=1} (w_i m_i P_i - w_i Q_i), P_i = sum_{j<i} w_j, Q_i = sum_{j<i} w_j m_j.
template <class WAt, class MAt, class DAt>
__device__ __forceinline__ double obj_distloss_ray(int n, int lane, WAt w_at, MAt m_at, DAt d_at) {
  double carry_w = 0.0, carry_wm = 0.0, acc = 0.0;
  for (int b = 0; b * 64 < n; ++b) {
    const int i = b * 64 + lane;
    const bool ok = i < n;
    const double w = ok ? w_at(i) : 0.0, m = ok ? m_at(i) : 0.0, d = ok ? d_at(i) : 0.0;
    const double iw = obj_scan_sum(w, lane), iwm = obj_scan_sum(w * m, lane);
    const double P = carry_w + iw - w, Q = carry_wm + iwm - w * m;
    acc += d * w * w * (1.0 / 3.0) + 2.0 * (w * m * P - w * Q);
    carry_w += __shfl(iw, 63);
    carry_wm += __shfl(iwm, 63);
  }
  return obj_wave_sum(acc);
}
// its gradient: dw_k = (2/3) d_k w_k + 2 [m_k (P_k - S_k) - (Q_k - T_k)], dm_k = 2 w_k (P_k - S_k), dd_k = w_k^2 / 3, all times `scale`;
// S_k = sum_{j>k} w_j = total - P_k - w_k, T_k likewise.  put(i, dw, dm, dd) stores element i.
template <class WAt, class MAt, class DAt, class Put>
__device__ __forceinline__ void obj_distloss_ray_bwd(int n, int lane, double scale, WAt w_at, MAt m_at, DAt d_at, Put put) {
  double tot_w = 0.0, tot_wm = 0.0;
  const bool one = n <= 64;  // a ray of one chunk: the totals are the last lane of the scans below
  if (!one) {
    for (int b = 0; b * 64 < n; ++b) {
      const int i = b * 64 + lane;
      const double w = i < n ? w_at(i) : 0.0, m = i < n ? m_at(i) : 0.0;
      tot_w += w;
      tot_wm += w * m;
    }
    tot_w = obj_wave_sum(tot_w);
    tot_wm = obj_wave_sum(tot_wm);
  }
  double carry_w = 0.0, carry_wm = 0.0;
  for (int b = 0; b * 64 < n; ++b) {
    const int i = b * 64 + lane;
    const bool ok = i < n;
    const double w = ok ? w_at(i) : 0.0, m = ok ? m_at(i) : 0.0, d = ok ? d_at(i) : 0.0;
    const double iw = obj_scan_sum(w, lane), iwm = obj_scan_sum(w * m, lane);
    if (one) {
      tot_w = __shfl(iw, 63);
      tot_wm = __shfl(iwm, 63);
    }
    const double P = carry_w + iw - w, Q = carry_wm + iwm - w * m;
    const double Sw = tot_w - (carry_w + iw), Swm = tot_wm - (carry_wm + iwm);
    if (ok) put(i, scale * ((2.0 / 3.0) * d * w + 2.0 * (m * (P - Sw) - (Q - Swm))), scale * 2.0 * w * (P - Sw), scale * w * w * (1.0 / 3.0));
    carry_w += __shfl(iw, 63);
    carry_wm += __shfl(iwm, 63);
  }
}

// the per-ray scalars both directions need: ratio = a / clamp(a + b, 1e-9), the static mask (train.py:400-414, :424-441)
struct ObjRay {
  double a, b, c, ratio, ssm, sm2;
};
__device__ __forceinline__ ObjRay obj_ray_scalars(double a, double b, double static_mask, double mref) {
  ObjRay q;
  q.a = a;
  q.b = b;
  q.c = fmax(a + b, 1e-9);
  q.ratio = a / q.c;
  q.ssm = (1.0 - static_mask) * mref * (1.0 - q.ratio);
  q.sm2 = q.ssm * (q.ratio < 0.1 ? 1.0 : 0.0);
  return q;
}

// ---- forward, per ray -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OBJ_THREADS) k_objective_rays(DynObjectiveParams p, double* __restrict__ rays, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * OBJ_RAYS_PER_WG + wave;
  double* sm = reinterpret_cast<double*>(dyn_smem);  // [OBJ_RAYS_PER_WG][OBJ_NRAY]
  double v[OBJ_NRAY];
#pragma unroll
  for (int k = 0; k < OBJ_NRAY; ++k) v[k] = 0.0;
  if (r < p.R) {  // (whole wavefronts)
    const int S = p.S;
    const long row = (long)r * S;
    double a = 0.0, b = 0.0, occ = 0.0;
    for (int i = lane; i < S; i += 64) {
      a += (double)p.weights_dy[row + i];
      b += (double)p.weights_st[row + i];
      occ += (double)p.occ_weights[row + i];
    }
    a = obj_wave_sum(a);
    b = obj_wave_sum(b);
    occ = obj_wave_sum(occ);
    // distortion (train.py:416-423): weights[:, :-1] against the midpoints and lengths of the S - 1 intervals of s_vals
    const float* w = p.weights + row;
    const float* sv = p.s_vals + row;
    const double dist = obj_distloss_ray(
        S - 1, lane, [&](int i) { return (double)w[i]; }, [&](int i) { return ((double)sv[i + 1] + (double)sv[i]) * 0.5; },
        [&](int i) { return (double)sv[i + 1] - (double)sv[i]; });
    if (lane == 0) {
      const double mref = p.mask_ref[r] ? 1.0 : 0.0, mm = (double)p.motion_mask[r];
      const double m_refdy = (p.mask_ref_dy[r] ? 1.0 : 0.0) * mm;
      const double fw_anc = (p.mask_anc[r] ? 1.0 : 0.0) * (double)p.owm_anc[r];
      const double fw_ancdy = (p.mask_anc_dy[r] ? 1.0 : 0.0) * mm * (double)p.owm_anc_dy[r];
      const ObjRay q = obj_ray_scalars(a, b, (double)p.static_mask[r], mref);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double t = (double)p.t_rgb[r * 3 + c];
        v[OBJ_N_REF] += obj_charb((double)p.rgb_ref[r * 3 + c], t) * mref;
        v[OBJ_N_ANC] += fw_anc * obj_charb((double)p.rgb_anc[r * 3 + c], t);
        v[OBJ_N_DYN] += obj_charb((double)p.rgb_dy[r * 3 + c], t) * (mref * mm);
        v[OBJ_N_REFDY] += obj_charb((double)p.rgb_ref_dy[r * 3 + c], t) * m_refdy;
        v[OBJ_N_ANCDY] += fw_ancdy * obj_charb((double)p.rgb_anc_dy[r * 3 + c], t);
        v[OBJ_N_ST] += obj_charb((double)p.rgb_static[r * 3 + c], t) * q.ssm;
      }
      v[OBJ_D_REF] = mref;
      v[OBJ_D_ANC] = fw_anc;
      v[OBJ_D_DYN] = mref * mm;
      v[OBJ_D_REFDY] = m_refdy;
      v[OBJ_D_ANCDY] = fw_ancdy;
      v[OBJ_D_ST] = q.ssm;
      v[OBJ_N_DISP] = fabs(1.0 / fmax((double)p.depth[r], 1e-2) - (double)p.t_disp[r]) * mref;
      for (int vw = 0; vw < p.NV; ++vw) {
        const long o = (long)vw * p.R + r;
        const double fm = mref * (double)p.t_masks[o];
        v[OBJ_N_FLOW] += (fabs((double)p.render_flows[o * 2] - (double)p.t_flows[o * 2]) +
                          fabs((double)p.render_flows[o * 2 + 1] - (double)p.t_flows[o * 2 + 1])) * fm;
        v[OBJ_D_FLOW] += fm;
      }
      v[OBJ_ENT] = -(q.ratio * log(q.ratio + 1e-9) + (1.0 - q.ratio) * log(1.0 - q.ratio + 1e-9));
      v[OBJ_DIST] = dist;
      v[OBJ_N_ST2] = fabs(a * q.sm2);
      v[OBJ_D_ST2] = q.sm2 + 1e-8;
      v[OBJ_D_OCC] = occ;
      rays[(long)r * 2] = a;
      rays[(long)r * 2 + 1] = b;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < OBJ_NRAY; ++k) sm[wave * OBJ_NRAY + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < OBJ_NRAY) {
    double s = 0.0;
    for (int wv = 0; wv < OBJ_RAYS_PER_WG; ++wv) s += sm[wv * OBJ_NRAY + threadIdx.x];
    partial[(long)blockIdx.x * OBJ_NRAY + threadIdx.x] = s;
  }
}

// ---- forward, per sample ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OBJ_THREADS) k_objective_samples(const float* __restrict__ pr, const float* __restrict__ pa,
                                                                   const float* __restrict__ ow, const float* __restrict__ sf, int T, long RS,
                                                                   int S, double* __restrict__ partial) {
  const long idx = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double cyc = 0.0, sabs = 0.0, st2 = 0.0, ssp = 0.0;
  if (idx < RS) {
    if (pr) {
      double d = 0.0;
      for (int t = 0; t < T; ++t) {
        const long o = ((long)t * RS + idx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) d += fabs((double)pr[o + c] - (double)pa[o + c]);
      }
      cyc = d * (double)ow[idx];
    }
    if (sf) {
      const bool inner = (int)(idx % S) < S - 1;  // has a neighbour along S
      double prev[3] = {0.0, 0.0, 0.0};
      for (int t = 0; t < 6; ++t) {
        const long o = ((long)t * RS + idx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double x = (double)sf[o + c];
          sabs += fabs(x);
          if (t > 0) st2 += (prev[c] - x) * (prev[c] - x);
          if (inner) ssp += fabs((double)sf[o + 3 + c] - x);
          prev[c] = x;
        }
      }
    }
  }
  cyc = obj_wave_sum(cyc);
  sabs = obj_wave_sum(sabs);
  st2 = obj_wave_sum(st2);
  ssp = obj_wave_sum(ssp);
  double* sm = reinterpret_cast<double*>(dyn_smem);  // [4 waves][OBJ_NSMP]
  if (lane == 0) {
    sm[wave * OBJ_NSMP + OBJ_N_CYC] = cyc;
    sm[wave * OBJ_NSMP + OBJ_SF_ABS] = sabs;
    sm[wave * OBJ_NSMP + OBJ_SF_T2] = st2;
    sm[wave * OBJ_NSMP + OBJ_SF_SP] = ssp;
  }
  __syncthreads();
  if (threadIdx.x < OBJ_NSMP) {
    double s = 0.0;
    for (int wv = 0; wv < OBJ_THREADS / 64; ++wv) s += sm[wv * OBJ_NSMP + threadIdx.x];
    partial[(long)blockIdx.x * OBJ_NSMP + threadIdx.x] = s;
  }
}

// ---- the fixed-order second stage -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double obj_column_sum(const double* __restrict__ part, long rows, int ncol, int col, int lane) {
  // lane l adds rows l, l + 64, ... in ascending order into four accumulators (row / 64 mod 4: four loads in flight instead of one
  // dependent chain), then ((s0 + s1) + (s2 + s3)) and the butterfly over the lanes: a fixed order, whatever the launch
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  long i = lane;
  for (; i + 192 < rows; i += 256) {
    s0 += part[i * ncol + col];
    s1 += part[(i + 64) * ncol + col];
    s2 += part[(i + 128) * ncol + col];
    s3 += part[(i + 192) * ncol + col];
  }
  if (i < rows) s0 += part[i * ncol + col];
  if (i + 64 < rows) s1 += part[(i + 64) * ncol + col];
  if (i + 128 < rows) s2 += part[(i + 128) * ncol + col];
  return obj_wave_sum((s0 + s1) + (s2 + s3));
}
__device__ __forceinline__ double obj_term(double k, double n, double d) { return k != 0.0 ? k * n / d : 0.0; }

#define OBJ_FINISH_THREADS 512
__global__ void __launch_bounds__(OBJ_FINISH_THREADS) k_objective_finish(DynObjectiveParams p, const double* __restrict__ pray, long nbr,
                                                                         const double* __restrict__ psmp, long nbs, double* __restrict__ coef,
                                                                         float* __restrict__ loss, float* __restrict__ logged) {
  // eight wavefronts share the OBJ_NRAY + OBJ_NSMP columns (a column is summed by ONE wavefront, so its order does not depend on the split)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* sm = reinterpret_cast<double*>(dyn_smem);  // [OBJ_NRAY + OBJ_NSMP]
  for (int k = wave; k < OBJ_NRAY + OBJ_NSMP; k += OBJ_FINISH_THREADS / 64) {
    const double v = k < OBJ_NRAY ? obj_column_sum(pray, nbr, OBJ_NRAY, k, lane) : obj_column_sum(psmp, nbs, OBJ_NSMP, k - OBJ_NRAY, lane);
    if (lane == 0) sm[k] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s[OBJ_NRAY], q[OBJ_NSMP];
#pragma unroll
  for (int k = 0; k < OBJ_NRAY; ++k) s[k] = sm[k];
#pragma unroll
  for (int k = 0; k < OBJ_NSMP; ++k) q[k] = sm[OBJ_NRAY + k];
  const double R = (double)p.R, S = (double)p.S;
  const double have_cyc = p.pts_traj_ref ? p.w_cycle : 0.0, have_reg = p.sf_seq ? p.w_reg : 0.0;
  double c[OBJ_NCOEF];
  c[OBJ_C_REF] = obj_term(p.k_rgb, 1.0, s[OBJ_D_REF] * 3.0 + 1e-6);
  c[OBJ_C_ANC] = obj_term(p.k_rgb, 1.0, s[OBJ_D_ANC] * 3.0 + 1e-8);
  c[OBJ_C_DYN] = obj_term(p.k_rgb_dyn, 1.0, s[OBJ_D_DYN] * 3.0 + 1e-6);
  c[OBJ_C_REFDY] = obj_term(p.k_rgb_dy, 1.0, s[OBJ_D_REFDY] * 3.0 + 1e-6);
  c[OBJ_C_ANCDY] = obj_term(p.k_rgb_dy, 1.0, s[OBJ_D_ANCDY] * 3.0 + 1e-8);
  c[OBJ_C_DISP] = obj_term(p.w_disp, 1.0, s[OBJ_D_REF] + 1e-8);
  c[OBJ_C_FLOW] = obj_term(p.w_flow, 1.0, s[OBJ_D_FLOW] * 2.0 + 1e-8);
  c[OBJ_C_CYC] = obj_term(have_cyc, 1.0, s[OBJ_D_OCC] * 3.0 * (double)p.T + 1e-8);
  c[OBJ_C_SFABS] = obj_term(have_reg, 1.0, 18.0 * R * S);
  c[OBJ_C_SFT] = obj_term(have_reg, 0.5, 15.0 * R * S);
  c[OBJ_C_SFSP] = obj_term(have_reg, 1.0, 18.0 * R * (S - 1.0));
  c[OBJ_C_ENT] = p.w_entropy / R;
  c[OBJ_C_DIST] = p.w_distortion / R;
  c[OBJ_C_ST] = obj_term(p.k_static, 1.0, s[OBJ_D_ST] * 3.0 + 1e-6);
  c[OBJ_C_ST2] = obj_term(p.k_static2, 1.0, s[OBJ_D_ST2]);
#pragma unroll
  for (int k = 0; k < OBJ_NCOEF; ++k) coef[k] = c[k];
  // the terms in train.py's order of addition (:443-452)
  const double rgb = ((c[OBJ_C_REF] * s[OBJ_N_REF] + c[OBJ_C_ANC] * s[OBJ_N_ANC]) + c[OBJ_C_DYN] * s[OBJ_N_DYN]) +
                     c[OBJ_C_REFDY] * s[OBJ_N_REFDY] + c[OBJ_C_ANCDY] * s[OBJ_N_ANCDY];
  const double cyc = c[OBJ_C_CYC] * q[OBJ_N_CYC];
  const double flow = c[OBJ_C_FLOW] * s[OBJ_N_FLOW];
  const double disp = c[OBJ_C_DISP] * s[OBJ_N_DISP];
  const double reg = c[OBJ_C_SFABS] * q[OBJ_SF_ABS] + c[OBJ_C_SFT] * q[OBJ_SF_T2] + c[OBJ_C_SFSP] * q[OBJ_SF_SP];
  const double ent = c[OBJ_C_ENT] * s[OBJ_ENT];
  const double dist = c[OBJ_C_DIST] * s[OBJ_DIST];
  const double stat = c[OBJ_C_ST] * s[OBJ_N_ST] + c[OBJ_C_ST2] * s[OBJ_N_ST2];
  const double total = rgb + cyc + flow + disp + reg + ent + dist + stat;
  loss[0] = (float)total;
  logged[0] = (float)total;
  logged[1] = (float)rgb;
  logged[2] = (float)cyc;
  logged[3] = (float)flow;
  logged[4] = (float)disp;
  logged[5] = (float)reg;
  logged[6] = (float)ent;
  logged[7] = (float)dist;
  logged[8] = (float)stat;
}

// ---- backward, per ray ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OBJ_THREADS) k_objective_rays_bwd(DynObjectiveParams p, DynObjectiveGrads g, const double* __restrict__ coef,
                                                                    const double* __restrict__ rays) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * OBJ_RAYS_PER_WG + (threadIdx.x >> 6);
  if (r >= p.R) return;  // (whole wavefronts; no workgroup barrier below)
  const int S = p.S;
  const long row = (long)r * S;
  const double G = (double)g.grad_loss[0];
  const double mref = p.mask_ref[r] ? 1.0 : 0.0, mm = (double)p.motion_mask[r];
  const ObjRay q = obj_ray_scalars(rays[(long)r * 2], rays[(long)r * 2 + 1], (double)p.static_mask[r], mref);
  if (lane < 3) {  // the colour cotangents, a lane per channel
    const int o = r * 3 + lane;
    const double t = (double)p.t_rgb[o];
    if (g.rgb_ref) g.rgb_ref[o] = (float)(G * coef[OBJ_C_REF] * mref * obj_dcharb((double)p.rgb_ref[o], t));
    if (g.rgb_dy) g.rgb_dy[o] = (float)(G * coef[OBJ_C_DYN] * (mref * mm) * obj_dcharb((double)p.rgb_dy[o], t));
    if (g.rgb_static) g.rgb_static[o] = (float)(G * coef[OBJ_C_ST] * q.ssm * obj_dcharb((double)p.rgb_static[o], t));
    if (g.rgb_ref_dy) g.rgb_ref_dy[o] = (float)(G * coef[OBJ_C_REFDY] * ((p.mask_ref_dy[r] ? 1.0 : 0.0) * mm) * obj_dcharb((double)p.rgb_ref_dy[o], t));
    if (g.rgb_anc) g.rgb_anc[o] = (float)(G * coef[OBJ_C_ANC] * ((p.mask_anc[r] ? 1.0 : 0.0) * (double)p.owm_anc[r]) * obj_dcharb((double)p.rgb_anc[o], t));
    if (g.rgb_anc_dy)
      g.rgb_anc_dy[o] = (float)(G * coef[OBJ_C_ANCDY] * ((p.mask_anc_dy[r] ? 1.0 : 0.0) * mm * (double)p.owm_anc_dy[r]) * obj_dcharb((double)p.rgb_anc_dy[o], t));
  }
  if (g.depth && lane == 3) {  // d |1 / clamp(z, 1e-2) - disp| : the clamp passes the gradient where z >= 1e-2
    const double z = (double)p.depth[r];
    const double zc = fmax(z, 1e-2);
    g.depth[r] = (float)(G * coef[OBJ_C_DISP] * mref * obj_sign(1.0 / zc - (double)p.t_disp[r]) * (z >= 1e-2 ? -1.0 / (zc * zc) : 0.0));
  }
  if (g.render_flows && lane >= 4 && lane < 4 + 2 * p.NV) {
    const int vw = (lane - 4) >> 1, c = (lane - 4) & 1;
    const long o = (long)vw * p.R + r;
    g.render_flows[o * 2 + c] = (float)(G * coef[OBJ_C_FLOW] * mref * (double)p.t_masks[o] * obj_sign((double)p.render_flows[o * 2 + c] - (double)p.t_flows[o * 2 + c]));
  }
  if (g.weights_dy || g.weights_st) {
    // entropy e(rho), rho = a / c, c = clamp(a + b, 1e-9): de/drho, drho/da = 1/c - [a+b >= 1e-9] a/c^2, drho/db = -[a+b >= 1e-9] a/c^2
    const double rho = q.ratio;
    const double de = -(log(rho + 1e-9) + rho / (rho + 1e-9) - log(1.0 - rho + 1e-9) - (1.0 - rho) / (1.0 - rho + 1e-9));
    const double thru = (q.a + q.b >= 1e-9) ? q.a / (q.c * q.c) : 0.0;
    const double ga = G * (coef[OBJ_C_ENT] * de * (1.0 / q.c - thru) + coef[OBJ_C_ST2] * obj_sign(q.a * q.sm2) * q.sm2);
    const double gb = G * coef[OBJ_C_ENT] * de * (-thru);
    for (int i = lane; i < S; i += 64) {
      if (g.weights_dy) g.weights_dy[row + i] = (float)ga;
      if (g.weights_st) g.weights_st[row + i] = (float)gb;
    }
  }
  if (g.weights) {
    const float* w = p.weights + row;
    const float* sv = p.s_vals + row;
    float* gw = g.weights + row;
    obj_distloss_ray_bwd(
        S - 1, lane, G * coef[OBJ_C_DIST], [&](int i) { return (double)w[i]; }, [&](int i) { return ((double)sv[i + 1] + (double)sv[i]) * 0.5; },
        [&](int i) { return (double)sv[i + 1] - (double)sv[i]; }, [&](int i, double dw, double, double) { gw[i] = (float)dw; });
    if (lane == 0) gw[S - 1] = 0.f;  // weights[:, -1] is not part of the loss
  }
}

// ---- backward, per sample ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OBJ_THREADS) k_objective_samples_bwd(const float* __restrict__ pr, const float* __restrict__ pa,
                                                                       const float* __restrict__ ow, const float* __restrict__ sf, int T,
                                                                       long RS, int S, const double* __restrict__ coef,
                                                                       const float* __restrict__ grad_loss, float* __restrict__ g_pr,
                                                                       float* __restrict__ g_pa, float* __restrict__ g_sf) {
  const long idx = (long)blockIdx.x * OBJ_THREADS + threadIdx.x;
  if (idx >= RS) return;
  const double G = (double)grad_loss[0];
  if (g_pr || g_pa) {
    const double k = G * coef[OBJ_C_CYC] * (double)ow[idx];
    for (int t = 0; t < T; ++t) {
      const long o = ((long)t * RS + idx) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = k * obj_sign((double)pr[o + c] - (double)pa[o + c]);
        if (g_pr) g_pr[o + c] = (float)d;
        if (g_pa) g_pa[o + c] = (float)(-d);
      }
    }
  }
  if (g_sf) {
    const int s = (int)(idx % S);
    const double k_abs = G * coef[OBJ_C_SFABS], k_t = G * coef[OBJ_C_SFT] * 2.0, k_sp = G * coef[OBJ_C_SFSP];
    double prev[3] = {0.0, 0.0, 0.0}, cur[3], nxt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) cur[c] = (double)sf[idx * 3 + c];
    for (int t = 0; t < 6; ++t) {
      const long o = ((long)t * RS + idx) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        nxt[c] = t < 5 ? (double)sf[o + RS * 3 + c] : 0.0;
        const double x = cur[c];
        double d = k_abs * obj_sign(x);
        // 0.5 mean (sf[t] - sf[t+1])^2: element t is the minuend of pair t and the subtrahend of pair t - 1
        d += k_t * ((t < 5 ? x - nxt[c] : 0.0) - (t > 0 ? prev[c] - x : 0.0));
        // mean |sf[s+1] - sf[s]|: element s is the minuend of pair s - 1 and the subtrahend of pair s
        d += k_sp * ((s > 0 ? obj_sign(x - (double)sf[o - 3 + c]) : 0.0) - (s < S - 1 ? obj_sign((double)sf[o + 3 + c] - x) : 0.0));
        g_sf[o + c] = (float)d;
        prev[c] = x;
        cur[c] = nxt[c];
      }
    }
  }
}

// ---- eff_distloss_native on its own -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(OBJ_THREADS) k_distloss(const float* __restrict__ w, long ld_w, const float* __restrict__ m, long ld_m,
                                                          const float* __restrict__ d, long ld_d, long R, int S, double* __restrict__ partial) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long r = (long)blockIdx.x * OBJ_RAYS_PER_WG + wave;
  double v = 0.0;
  if (r < R) {
    const float *wr = w + r * ld_w, *mr = m + r * ld_m, *dr = d + r * ld_d;
    v = obj_distloss_ray(S, lane, [&](int i) { return (double)wr[i]; }, [&](int i) { return (double)mr[i]; }, [&](int i) { return (double)dr[i]; });
  }
  double* sm = reinterpret_cast<double*>(dyn_smem);
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
}
__global__ void __launch_bounds__(64) k_distloss_finish(const double* __restrict__ partial, long n, long R, float* __restrict__ loss) {
  const double s = obj_column_sum(partial, n, 1, 0, threadIdx.x);
  if (threadIdx.x == 0) loss[0] = (float)(s / (double)R);
}
__global__ void __launch_bounds__(OBJ_THREADS) k_distloss_bwd(const float* __restrict__ w, long ld_w, const float* __restrict__ m, long ld_m,
                                                              const float* __restrict__ d, long ld_d, long R, int S,
                                                              const float* __restrict__ grad_loss, float* __restrict__ dw, float* __restrict__ dm,
                                                              float* __restrict__ dd) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * OBJ_RAYS_PER_WG + (threadIdx.x >> 6);
  if (r >= R) return;
  const float *wr = w + r * ld_w, *mr = m + r * ld_m, *dr = d + r * ld_d;
  const long row = r * S;
  obj_distloss_ray_bwd(
      S, lane, (double)grad_loss[0] / (double)R, [&](int i) { return (double)wr[i]; }, [&](int i) { return (double)mr[i]; },
      [&](int i) { return (double)dr[i]; },
      [&](int i, double gw, double gm, double gd) {
        if (dw) dw[row + i] = (float)gw;
        if (dm) dm[row + i] = (float)gm;
        if (dd) dd[row + i] = (float)gd;
      });
}

// ---- C ABI --------------------------------------------------------------------------------------------------------------------------------
extern "C" size_t dyn_objective_workspace_bytes(int R, int S) {
  if (R <= 0 || S < 2 || (long)R * S > (1L << 28)) return 0;
  return obj_layout(R, S).bytes;
}

static int obj_check(const DynObjectiveParams* p, const char* who) {
  DYN_REQUIRE(p, "%s: null params", who);
  DYN_REQUIRE(p->R > 0 && p->S >= 2, "%s: R > 0 and S >= 2 (the spatial smoothness term is a mean over S - 1 elements)", who);
  DYN_REQUIRE((long)p->R * p->S <= (1L << 28), "%s: R * S must not exceed 2^28", who);
  DYN_REQUIRE(p->NV >= 0 && p->NV <= 6, "%s: at most 6 flow views", who);
  DYN_REQUIRE(p->T >= 0, "%s: T < 0", who);
  DYN_REQUIRE(p->t_rgb && p->t_disp && p->motion_mask && p->static_mask && p->rgb_ref && p->rgb_dy && p->rgb_static && p->depth && p->weights &&
                  p->weights_dy && p->weights_st && p->s_vals && p->mask_ref && p->rgb_ref_dy && p->rgb_anc && p->rgb_anc_dy && p->owm_anc &&
                  p->owm_anc_dy && p->mask_ref_dy && p->mask_anc && p->mask_anc_dy && p->occ_weights,
              "%s: a per-ray input is NULL", who);
  DYN_REQUIRE(p->NV == 0 || (p->t_flows && p->t_masks && p->render_flows), "%s: NV > 0 without flows", who);
  DYN_REQUIRE((p->pts_traj_ref != nullptr) == (p->pts_traj_anchor != nullptr), "%s: pts_traj_ref and pts_traj_anchor come together", who);
  DYN_REQUIRE(!p->pts_traj_ref || p->T > 0, "%s: trajectories with T = 0", who);
  DYN_REQUIRE(p->workspace && p->workspace_bytes >= obj_layout(p->R, p->S).bytes && (size_t)p->workspace % 8 == 0,
              "%s: workspace of dyn_objective_workspace_bytes(R, S) bytes, 8-byte aligned", who);
  return 0;
}

extern "C" int dyn_objective_fwd(const DynObjectiveParams* p, float* loss, float* logged, void* stream) {
  if (int rc = obj_check(p, "dyn_objective_fwd")) return rc;
  DYN_REQUIRE(loss && logged, "dyn_objective_fwd: null outputs");
  const ObjLayout L = obj_layout(p->R, p->S);
  char* ws = (char*)p->workspace;
  double *coef = (double*)ws, *rays = (double*)(ws + L.off_rays), *pray = (double*)(ws + L.off_pray), *psmp = (double*)(ws + L.off_psmp);
  hipStream_t st = (hipStream_t)stream;
  DYN_LAUNCH(DYN_K_OBJECTIVE_FWD, "k_objective_rays", k_objective_rays, dim3((unsigned)L.nbr), dim3(OBJ_THREADS),
             OBJ_RAYS_PER_WG * OBJ_NRAY * sizeof(double), st, *p, rays, pray);
  const bool samples = p->pts_traj_ref || p->sf_seq;
  if (samples)
    DYN_LAUNCH(DYN_K_OBJECTIVE_FWD, "k_objective_samples", k_objective_samples, dim3((unsigned)L.nbs), dim3(OBJ_THREADS),
               (OBJ_THREADS / 64) * OBJ_NSMP * sizeof(double), st, p->pts_traj_ref, p->pts_traj_anchor, p->occ_weights, p->sf_seq, p->T,
               (long)p->R * p->S, p->S, psmp);
  DYN_LAUNCH(DYN_K_OBJECTIVE_FWD, "k_objective_finish", k_objective_finish, dim3(1), dim3(OBJ_FINISH_THREADS),
             (OBJ_NRAY + OBJ_NSMP) * sizeof(double), st, *p, (const double*)pray, L.nbr,
             (const double*)psmp, samples ? L.nbs : 0L, coef, loss, logged);
  return 0;
}

extern "C" int dyn_objective_bwd(const DynObjectiveParams* p, const DynObjectiveGrads* g, void* stream) {
  if (int rc = obj_check(p, "dyn_objective_bwd")) return rc;
  DYN_REQUIRE(g && g->grad_loss, "dyn_objective_bwd: null cotangents / grad_loss");
  DYN_REQUIRE(!(g->pts_traj_ref || g->pts_traj_anchor) || p->pts_traj_ref, "dyn_objective_bwd: a trajectory cotangent without the trajectories");
  DYN_REQUIRE(!g->sf_seq || p->sf_seq, "dyn_objective_bwd: a cotangent of sf_seq without sf_seq");
  const ObjLayout L = obj_layout(p->R, p->S);
  char* ws = (char*)p->workspace;
  const double *coef = (const double*)ws, *rays = (const double*)(ws + L.off_rays);
  hipStream_t st = (hipStream_t)stream;
  if (g->rgb_ref || g->rgb_dy || g->rgb_static || g->rgb_ref_dy || g->rgb_anc || g->rgb_anc_dy || g->depth || g->render_flows || g->weights ||
      g->weights_dy || g->weights_st)
    DYN_LAUNCH(DYN_K_OBJECTIVE_BWD, "k_objective_rays_bwd", k_objective_rays_bwd, dim3((unsigned)L.nbr), dim3(OBJ_THREADS), 0, st, *p, *g, coef,
               rays);
  if (g->pts_traj_ref || g->pts_traj_anchor || g->sf_seq)
    DYN_LAUNCH(DYN_K_OBJECTIVE_BWD, "k_objective_samples_bwd", k_objective_samples_bwd, dim3((unsigned)L.nbs), dim3(OBJ_THREADS), 0, st,
               p->pts_traj_ref, p->pts_traj_anchor, p->occ_weights, p->sf_seq, p->T, (long)p->R * p->S, p->S, coef, g->grad_loss, g->pts_traj_ref,
               g->pts_traj_anchor, g->sf_seq);
  return 0;
}

extern "C" long dyn_distloss_partials(long R) { return R > 0 ? (R + OBJ_RAYS_PER_WG - 1) / OBJ_RAYS_PER_WG : 0; }

extern "C" int dyn_distloss_fwd(const float* w, long ld_w, const float* m, long ld_m, const float* interval, long ld_i, long R, int S,
                                double* partial, float* loss, void* stream) {
  DYN_REQUIRE(w && m && interval && partial && loss && R > 0 && S > 0 && ld_w >= S && ld_m >= S && ld_i >= S, "dyn_distloss_fwd: bad arguments");
  DYN_REQUIRE(R <= (1L << 30), "dyn_distloss_fwd: at most 2^30 rays");
  const long nb = dyn_distloss_partials(R);
  DYN_LAUNCH(DYN_K_OBJECTIVE_FWD, "k_distloss", k_distloss, dim3((unsigned)nb), dim3(OBJ_THREADS), OBJ_RAYS_PER_WG * sizeof(double),
             (hipStream_t)stream, w, ld_w, m, ld_m, interval, ld_i, R, S, partial);
  DYN_LAUNCH(DYN_K_OBJECTIVE_FWD, "k_distloss_finish", k_distloss_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)partial, nb, R,
             loss);
  return 0;
}

extern "C" int dyn_distloss_bwd(const float* w, long ld_w, const float* m, long ld_m, const float* interval, long ld_i, long R, int S,
                                const float* grad_loss, float* dw, float* dm, float* dinterval, void* stream) {
  DYN_REQUIRE(w && m && interval && grad_loss && R > 0 && S > 0 && ld_w >= S && ld_m >= S && ld_i >= S, "dyn_distloss_bwd: bad arguments");
  DYN_REQUIRE(R <= (1L << 30), "dyn_distloss_bwd: at most 2^30 rays");
  if (!dw && !dm && !dinterval) return 0;
  DYN_LAUNCH(DYN_K_OBJECTIVE_BWD, "k_distloss_bwd", k_distloss_bwd, dim3((unsigned)dyn_distloss_partials(R)), dim3(OBJ_THREADS), 0,
             (hipStream_t)stream, w, ld_w, m, ld_m, interval, ld_i, R, S, grad_loss, dw, dm, dinterval);
  return 0;
}
