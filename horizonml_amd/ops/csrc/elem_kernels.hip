// BatchNorm / pooling / classifier / loss / optimizer kernels for gfx950.
// All activation tensors are bf16 NHWC (flattened [M][C], channels innermost,
// coalesced along C); statistics and parameters are f32.
#include <cstdio>

#include "common.h"

// ------------------------------------------------------------- BN forward --
// y = gamma*(x-mean)*invstd + beta  [+ residual] [ReLU]
// Training: mean/var come from the conv epilogue's (Σy, Σy²) in `stats`;
// block 0 additionally writes save_mean/save_invstd and updates running
// stats.  Eval: running stats are used and nothing is written back.
// F32SRC (split-K conv path): x is the f32 workspace; the bf16 convout for
// backward is emitted here (`convout`) — the cast rides the same pass.
// V8 layout (C % 8 == 0, the universal case here): each thread handles 8
// consecutive channels of one row — 16-byte loads/stores and 8-deep ILP
// instead of one 2-byte element per thread (measured ~2x on these
// latency-bound shapes).
union F8 {
  float4 q[2];
  float f[8];
};

DEV F8 load_f8(const float* p) {
  F8 v;
  v.q[0] = *(const float4*)p;
  v.q[1] = *(const float4*)(p + 4);
  return v;
}

// ACT/TRAIN compile-time (mirrors k_bn_bwd_apply's MASK): the runtime
// branches kept ~390-instruction specialized loops alive; templated the
// V8 loop is lean and the eval path drops out of training kernels.
template <bool F32SRC, int ACT, bool TRAIN>
__global__ __launch_bounds__(256) void k_bn_apply(
    const void* __restrict__ xv, const bf16* __restrict__ res,
    bf16* __restrict__ y, bf16* __restrict__ convout,
    const float* __restrict__ stats,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float* __restrict__ save_mean, float* __restrict__ save_invstd,
    long M, int C, float momentum, float eps, int nsplit) {
  const long slab = M * (long)C;
  const bf16* xb = (const bf16*)xv;
  const float* xf = (const float*)xv;
  const float invM = 1.f / (float)M;
  if (TRAIN && blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float mean = stats[c] * invM;
      float var = fmaxf(stats[C + c] * invM - mean * mean, 0.f);
      save_mean[c] = mean;
      save_invstd[c] = rsqrtf(var + eps);
      // unbiased running var like torch.nn.BatchNorm2d
      float ub = (M > 1) ? var * (float)M / (float)(M - 1) : var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * ub;
    }
  }
  if (C % 8 != 0) {  // scalar fallback for off-grid channel counts
    long total = M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
      int c = (int)(i % C);
      float mean, invstd;
      if (TRAIN) {
        mean = stats[c] * invM;
        float var = fmaxf(stats[C + c] * invM - mean * mean, 0.f);
        invstd = rsqrtf(var + eps);
      } else {
        mean = running_mean[c];
        invstd = rsqrtf(running_var[c] + eps);
      }
      float xi;
      if (F32SRC) {
        xi = xf[i];
        for (int z = 1; z < nsplit; z++) xi += xf[z * slab + i];
      } else {
        xi = b2f(xb[i]);
      }
      if (F32SRC && convout != nullptr) convout[i] = f2b(xi);
      float v = (xi - mean) * invstd * gamma[c] + beta[c];
      if (res != nullptr) v += b2f(res[i]);
      if (ACT == 1) v = fmaxf(v, 0.f);
      else if (ACT == 2) v = fminf(fmaxf(v, 0.f), 6.f);
      y[i] = f2b(v);
    }
    return;
  }
  long total8 = M * C / 8;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total8;
       t += (long)gridDim.x * blockDim.x) {
    long i = t * 8;
    int c0 = (int)(i % C);
    F8 xi;
    if (F32SRC) {
      xi = load_f8(xf + i);
      for (int z = 1; z < nsplit; z++) {
        F8 w = load_f8(xf + z * slab + i);
#pragma unroll
        for (int e = 0; e < 8; e++) xi.f[e] += w.f[e];
      }
    } else {
      V8 xv8;
      xv8.u = *(const uint4*)(xb + i);
#pragma unroll
      for (int e = 0; e < 8; e++) xi.f[e] = b2f(xv8.e[e]);
    }
    if (F32SRC && convout != nullptr) {
      V8 co;
#pragma unroll
      for (int e = 0; e < 8; e++) co.e[e] = f2b(xi.f[e]);
      *(uint4*)(convout + i) = co.u;
    }
    F8 g8 = load_f8(gamma + c0), b8 = load_f8(beta + c0);
    F8 mean8, istd8;
    if (TRAIN) {
      F8 s1 = load_f8(stats + c0), s2 = load_f8(stats + C + c0);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        mean8.f[e] = s1.f[e] * invM;
        float var = fmaxf(s2.f[e] * invM - mean8.f[e] * mean8.f[e], 0.f);
        istd8.f[e] = rsqrtf(var + eps);
      }
    } else {
      F8 rm = load_f8(running_mean + c0), rv = load_f8(running_var + c0);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        mean8.f[e] = rm.f[e];
        istd8.f[e] = rsqrtf(rv.f[e] + eps);
      }
    }
    V8 r8;
    if (res != nullptr) r8.u = *(const uint4*)(res + i);
    V8 out;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float v = (xi.f[e] - mean8.f[e]) * istd8.f[e] * g8.f[e] + b8.f[e];
      if (res != nullptr) v += b2f(r8.e[e]);
      if (ACT == 1) v = fmaxf(v, 0.f);
      else if (ACT == 2) v = fminf(fmaxf(v, 0.f), 6.f);  // ReLU6
      out.e[e] = f2b(v);
    }
    *(uint4*)(y + i) = out.u;
  }
}

// c-blocked BN forward apply (the reduce kernels' slab geometry): each
// block owns a <=512-channel slab x m-chunk, so per-channel mean/invstd/
// gamma/beta fold into registers ONCE per block and the m-loop body is
// load -> 8 fma -> store.  The flat elementwise k_bn_apply recomputed the
// channel stats (incl. 8 precise rsqrtf) for EVERY 8-element tile —
// ~350-instruction loops, ~1.6x off the HBM roofline at r50@224.
template <bool F32SRC, int ACT, bool TRAIN>
__global__ __launch_bounds__(256) void k_bn_apply_v8(
    const void* __restrict__ xv, const bf16* __restrict__ res,
    bf16* __restrict__ y, bf16* __restrict__ convout,
    const float* __restrict__ stats,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float* __restrict__ save_mean, float* __restrict__ save_invstd,
    long M, int C, float momentum, float eps, int nsplit, long mchunk,
    int cslab) {
  const long slab = M * (long)C;
  const bf16* xb = (const bf16*)xv;
  const float* xf = (const float*)xv;
  const float invM = 1.f / (float)M;
  if (TRAIN && blockIdx.x == 0 && blockIdx.y == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float mean = stats[c] * invM;
      float var = fmaxf(stats[C + c] * invM - mean * mean, 0.f);
      save_mean[c] = mean;
      save_invstd[c] = rsqrtf(var + eps);
      float ub = (M > 1) ? var * (float)M / (float)(M - 1) : var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * ub;
    }
  }
  const int cbeg = blockIdx.x * cslab;
  const int lpr = cslab >> 3;
  const int mstep = 256 / lpr;
  const int tid = threadIdx.x;
  if (tid >= mstep * lpr) return;
  const int th_c = cbeg + (tid % lpr) * 8;
  const int th_m = tid / lpr;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float ga[8], be[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    int c = th_c + e;
    float mean, istd;
    if (TRAIN) {
      mean = stats[c] * invM;
      float var = fmaxf(stats[C + c] * invM - mean * mean, 0.f);
      istd = rsqrtf(var + eps);
    } else {
      mean = running_mean[c];
      istd = rsqrtf(running_var[c] + eps);
    }
    ga[e] = gamma[c] * istd;
    be[e] = beta[c] - mean * ga[e];   // y = ga*x + be  [+res] [act]
  }
  for (long m = mbeg + th_m; m < mend; m += mstep) {
    const long i = m * C + th_c;
    float v[8];
    if (F32SRC) {
#pragma unroll
      for (int q = 0; q < 8; q += 4)
        *(float4*)&v[q] = *(const float4*)(xf + i + q);
      for (int z = 1; z < nsplit; z++)
#pragma unroll
        for (int q = 0; q < 8; q += 4) {
          float4 w = *(const float4*)(xf + z * slab + i + q);
          v[q] += w.x; v[q + 1] += w.y; v[q + 2] += w.z; v[q + 3] += w.w;
        }
      if (convout != nullptr) {
        V8 co;
#pragma unroll
        for (int e = 0; e < 8; e++) co.e[e] = f2b(v[e]);
        *(uint4*)(convout + i) = co.u;
      }
    } else {
      V8 x8;
      x8.u = *(const uint4*)(xb + i);
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] = b2f(x8.e[e]);
    }
    V8 r8, out;
    if (res != nullptr) r8.u = *(const uint4*)(res + i);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float t = fmaf(ga[e], v[e], be[e]);
      if (res != nullptr) t += b2f(r8.e[e]);
      if (ACT == 1) t = fmaxf(t, 0.f);
      else if (ACT == 2) t = fminf(fmaxf(t, 0.f), 6.f);  // ReLU6
      out.e[e] = f2b(t);
    }
    *(uint4*)(y + i) = out.u;
  }
}

// Deterministic per-channel (Σx, Σx²) over a bf16 [M][C] tensor: ONE
// block per 64 channels, fixed-order serial m-loop per lane + ordered LDS
// reduce — no atomics, bitwise-reproducible (deterministic mode).
__global__ __launch_bounds__(256) void k_stats_bf16_det(
    const bf16* __restrict__ x, float* __restrict__ stats, long M, int C) {
  __shared__ float s1[4][64];
  __shared__ float s2[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    for (long m = mlane; m < M; m += 4) {
      float v = b2f(x[m * C + c]);
      a1 += v;
      a2 += v * v;
    }
  }
  s1[mlane][threadIdx.x & 63] = a1;
  s2[mlane][threadIdx.x & 63] = a2;
  __syncthreads();
  if (mlane == 0 && c < C) {
    stats[c] = s1[0][threadIdx.x] + s1[1][threadIdx.x] +
               s1[2][threadIdx.x] + s1[3][threadIdx.x];
    stats[C + c] = s2[0][threadIdx.x] + s2[1][threadIdx.x] +
                   s2[2][threadIdx.x] + s2[3][threadIdx.x];
  }
}

// Per-channel (Σx, Σx²) over `nsplit` stacked f32 [M][C] slabs (split-K
// conv path — slabs are summed here).  grid: (cdiv(C,64), msplit);
// stats must be pre-zeroed.
__global__ __launch_bounds__(256) void k_stats_reduce(
    const float* __restrict__ x, float* __restrict__ stats, long M, int C,
    long mchunk, int nsplit) {
  __shared__ float s1[4][64];
  __shared__ float s2[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min((long)M, mbeg + mchunk);
  const long slab = (long)M * C;
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    for (long m = mbeg + mlane; m < mend; m += 4) {
      float v = 0.f;
      for (int z = 0; z < nsplit; z++) v += x[z * slab + m * C + c];
      a1 += v;
      a2 += v * v;
    }
  }
  s1[mlane][threadIdx.x & 63] = a1;
  s2[mlane][threadIdx.x & 63] = a2;
  __syncthreads();
  if (mlane == 0 && c < C) {
    float t1 = s1[0][threadIdx.x] + s1[1][threadIdx.x] + s1[2][threadIdx.x] +
               s1[3][threadIdx.x];
    float t2 = s2[0][threadIdx.x] + s2[1][threadIdx.x] + s2[2][threadIdx.x] +
               s2[3][threadIdx.x];
    atomicAdd(&stats[c], t1);
    atomicAdd(&stats[C + c], t2);
  }
}

// Σ over nsplit f32 slabs -> bf16 elementwise (split-K dgrad output);
// V8 per thread (n % 8 == 0 for NHWC C%8 tensors).
__global__ __launch_bounds__(256) void k_cast_f32_bf16(
    const float* __restrict__ src, bf16* __restrict__ dst, long n,
    int nsplit, int accum) {
  if (n % 8 != 0) {  // scalar path (slab stride would misalign float4)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (long)gridDim.x * blockDim.x) {
      float v = src[i];
      for (int z = 1; z < nsplit; z++) v += src[(long)z * n + i];
      if (accum) v += b2f(dst[i]);
      dst[i] = f2b(v);
    }
    return;
  }
  long total8 = n / 8;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total8;
       t += (long)gridDim.x * blockDim.x) {
    long i = t * 8;
    F8 v = load_f8(src + i);
    for (int z = 1; z < nsplit; z++) {
      F8 w = load_f8(src + (long)z * n + i);
#pragma unroll
      for (int e = 0; e < 8; e++) v.f[e] += w.f[e];
    }
    V8 out;
    if (accum) {
      V8 d;
      d.u = *(const uint4*)(dst + i);
#pragma unroll
      for (int e = 0; e < 8; e++) out.e[e] = f2b(v.f[e] + b2f(d.e[e]));
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) out.e[e] = f2b(v.f[e]);
    }
    *(uint4*)(dst + i) = out.u;
  }
}

// Fused split-dgrad slab-sum + upstream BN-backward reduce: while summing
// the dgrad slabs into dy (bf16), also accumulate the UPSTREAM conv's
// per-channel Σdz and Σ(dz·xhat) — its k_bnact_bwd_reduce launch is then
// skipped entirely, and the sums use the unrounded f32 dy (closer to the
// fp32 reference than the two-kernel version).  accum: dy accumulates into
// dst (residual junction).  grid: (cdiv(C,64), msplit) like the reduce.
__global__ __launch_bounds__(256) void k_cast_bnact(
    const float* __restrict__ src, bf16* __restrict__ dst, long M, int C,
    int nsplit, int accum, const bf16* __restrict__ x_up,
    const bf16* __restrict__ y_up, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sum_dz,
    float* __restrict__ sum_dzx, int mask_mode, long mchunk) {
  __shared__ float sdz[4][64];
  __shared__ float sdzx[4][64];
  const long n = M * (long)C;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min((long)M, mbeg + mchunk);
  float a_dz = 0.f, a_dzx = 0.f;
  if (c < C) {
    const float mean = save_mean[c], invstd = save_invstd[c];
    const float ga = gamma[c] * invstd;
    const float gb = beta[c] - mean * ga;
    for (long m = mbeg + mlane; m < mend; m += 4) {
      long i = m * C + c;
      float v = src[i];
      for (int z = 1; z < nsplit; z++) v += src[z * n + i];
      if (accum) v += b2f(dst[i]);
      dst[i] = f2b(v);
      float g = v;
      float xv = b2f(x_up[i]);
      if (mask_mode == 1) {
        if (b2f(y_up[i]) <= 0.f) g = 0.f;
      } else if (mask_mode == 2) {
        if (fmaf(ga, xv, gb) <= 0.f) g = 0.f;
      } else if (mask_mode == 3) {
        float yv = b2f(y_up[i]);
        if (yv <= 0.f || yv >= 6.f) g = 0.f;
      } else if (mask_mode == 4) {
        float bn = fmaf(ga, xv, gb);
        if (bn <= 0.f || bn >= 6.f) g = 0.f;
      }
      a_dz += g;
      a_dzx += g * (xv - mean) * invstd;
    }
  }
  sdz[mlane][threadIdx.x & 63] = a_dz;
  sdzx[mlane][threadIdx.x & 63] = a_dzx;
  __syncthreads();
  if (mlane == 0 && c < C) {
    atomicAdd(&sum_dz[c], sdz[0][threadIdx.x] + sdz[1][threadIdx.x] +
                              sdz[2][threadIdx.x] + sdz[3][threadIdx.x]);
    atomicAdd(&sum_dzx[c], sdzx[0][threadIdx.x] + sdzx[1][threadIdx.x] +
                               sdzx[2][threadIdx.x] + sdzx[3][threadIdx.x]);
  }
}

// Vectorized (8 channels per lane, dwordx4) variants of the BN-backward
// reduce pair.  The scalar kernels stream the big [M,C] activations with
// 2-byte per-lane loads (128 B per wave-instruction) and ran ~13× off the
// HBM roofline at ResNet50@224 shapes (r50_224_pmc_mfma.txt: 1.9 ms/step
// in k_bnact_bwd_reduce alone); here each lane owns 8 consecutive
// channels, every load is a 16-byte dwordx4, and the whole C extent fits
// one block (C ≤ 2048), partial sums LDS-reduced across the block's
// m-lanes before one atomicAdd per channel.
// cslab: channels handled per block (blockIdx.x indexes slabs of the C
// extent).  cslab == C reproduces the original single-slab kernel; for
// C > 512 the launcher slices C into <=512-channel slabs so each block
// keeps >=4 m-rows in flight (full-C blocks at C=2048 had mstep=1 and
// lost to the scalar kernel at small M — dispatch-rule comment below).
template <int MASK>
__global__ __launch_bounds__(256) void k_bnact_bwd_reduce_v8(
    const bf16* __restrict__ dy, const bf16* __restrict__ yout,
    const bf16* __restrict__ x, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sum_dz,
    float* __restrict__ sum_dzx, long M, int C, long mchunk, int cslab) {
  // MASK compile-time: runtime mask branches in this 8-wide unrolled body
  // compiled to ~630 instructions per iteration (measured 45 GB/s)
  __shared__ float sdz[256][8];
  __shared__ float sdzx[256][8];
  const int cbeg = blockIdx.x * cslab;
  const int lpr = cslab >> 3;        // lanes per m-row
  const int mstep = 256 / lpr;       // m rows in flight per block
  const int active = mstep * lpr;
  const int tid = threadIdx.x;
  const int th_c = cbeg + (tid % lpr) * 8;
  const int th_m = tid / lpr;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float adz[8] = {}, adzx[8] = {}, mean[8], invstd[8], ga[8], gb[8];
  if (tid < active) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
      mean[e] = save_mean[th_c + e];
      invstd[e] = save_invstd[th_c + e];
      ga[e] = gamma[th_c + e] * invstd[e];
      gb[e] = beta[th_c + e] - mean[e] * ga[e];
    }
    for (long m = mbeg + th_m; m < mend; m += mstep) {
      V8 dv, xv8, yv8;
      dv.u = *(const uint4*)(dy + m * C + th_c);
      xv8.u = *(const uint4*)(x + m * C + th_c);
      if (MASK == 1 || MASK == 3)
        yv8.u = *(const uint4*)(yout + m * C + th_c);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float g = b2f(dv.e[e]);
        float xe = b2f(xv8.e[e]);
        if (MASK == 1) {
          if (b2f(yv8.e[e]) <= 0.f) g = 0.f;
        } else if (MASK == 2) {
          if (fmaf(ga[e], xe, gb[e]) <= 0.f) g = 0.f;
        } else if (MASK == 3) {
          float yv = b2f(yv8.e[e]);
          if (yv <= 0.f || yv >= 6.f) g = 0.f;
        } else if (MASK == 4) {
          float bn = fmaf(ga[e], xe, gb[e]);
          if (bn <= 0.f || bn >= 6.f) g = 0.f;
        }
        adz[e] += g;
        adzx[e] += g * (xe - mean[e]) * invstd[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    sdz[tid][e] = adz[e];
    sdzx[tid][e] = adzx[e];
  }
  __syncthreads();
  // wave-parallel channel reduction: flat LDS index j*C + c walks the
  // [m-lane][channel] partials; one lane per channel, ONE coalesced
  // atomic instruction per wave per array (the per-e unrolled epilogue
  // serialized ~0.2 us of LDS latency + 16 atomic issues per block)
  const float* S1 = &sdz[0][0];
  const float* S2 = &sdzx[0][0];
  for (int c = tid; c < cslab; c += 256) {
    float r1 = 0.f, r2 = 0.f;
    for (int j = 0; j < mstep; j++) {
      r1 += S1[j * cslab + c];
      r2 += S2[j * cslab + c];
    }
    atomicAdd(&sum_dz[cbeg + c], r1);
    atomicAdd(&sum_dzx[cbeg + c], r2);
  }
}

// Vectorized split-dgrad slab-sum + upstream BN reduce (k_cast_bnact's
// access pattern, 8 channels per lane — see k_bnact_bwd_reduce_v8).
template <int MASK>
__global__ __launch_bounds__(256) void k_cast_bnact_v8(
    const float* __restrict__ src, bf16* __restrict__ dst, long M, int C,
    int nsplit, int accum, const bf16* __restrict__ x_up,
    const bf16* __restrict__ y_up, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sum_dz,
    float* __restrict__ sum_dzx, long mchunk, int cslab) {
  __shared__ float sdz[256][8];
  __shared__ float sdzx[256][8];
  const long n = M * (long)C;
  const int cbeg = blockIdx.x * cslab;
  const int lpr = cslab >> 3;
  const int mstep = 256 / lpr;
  const int active = mstep * lpr;
  const int tid = threadIdx.x;
  const int th_c = cbeg + (tid % lpr) * 8;
  const int th_m = tid / lpr;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float adz[8] = {}, adzx[8] = {}, mean[8], invstd[8], ga[8], gb[8];
  if (tid < active) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
      mean[e] = save_mean[th_c + e];
      invstd[e] = save_invstd[th_c + e];
      ga[e] = gamma[th_c + e] * invstd[e];
      gb[e] = beta[th_c + e] - mean[e] * ga[e];
    }
    for (long m = mbeg + th_m; m < mend; m += mstep) {
      const long i = m * C + th_c;
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; q += 4)
        *(float4*)&v[q] = *(const float4*)(src + i + q);
      for (int z = 1; z < nsplit; z++)
#pragma unroll
        for (int q = 0; q < 8; q += 4) {
          float4 w = *(const float4*)(src + z * n + i + q);
          v[q] += w.x; v[q + 1] += w.y; v[q + 2] += w.z; v[q + 3] += w.w;
        }
      V8 out, xv8, yv8;
      xv8.u = *(const uint4*)(x_up + i);
      if (MASK == 1 || MASK == 3)
        yv8.u = *(const uint4*)(y_up + i);
      if (accum) {
        V8 d;
        d.u = *(const uint4*)(dst + i);
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] += b2f(d.e[e]);
      }
#pragma unroll
      for (int e = 0; e < 8; e++) {
        out.e[e] = f2b(v[e]);
        float g = v[e];
        float xe = b2f(xv8.e[e]);
        if (MASK == 1) {
          if (b2f(yv8.e[e]) <= 0.f) g = 0.f;
        } else if (MASK == 2) {
          if (fmaf(ga[e], xe, gb[e]) <= 0.f) g = 0.f;
        } else if (MASK == 3) {
          float yv = b2f(yv8.e[e]);
          if (yv <= 0.f || yv >= 6.f) g = 0.f;
        } else if (MASK == 4) {
          float bn = fmaf(ga[e], xe, gb[e]);
          if (bn <= 0.f || bn >= 6.f) g = 0.f;
        }
        adz[e] += g;
        adzx[e] += g * (xe - mean[e]) * invstd[e];
      }
      *(uint4*)(dst + i) = out.u;
    }
  }
#pragma unroll
  for (int e = 0; e < 8; e++) {
    sdz[tid][e] = adz[e];
    sdzx[tid][e] = adzx[e];
  }
  __syncthreads();
  // wave-parallel channel reduction: flat LDS index j*C + c walks the
  // [m-lane][channel] partials; one lane per channel, ONE coalesced
  // atomic instruction per wave per array (the per-e unrolled epilogue
  // serialized ~0.2 us of LDS latency + 16 atomic issues per block)
  const float* S1 = &sdz[0][0];
  const float* S2 = &sdzx[0][0];
  for (int c = tid; c < cslab; c += 256) {
    float r1 = 0.f, r2 = 0.f;
    for (int j = 0; j < mstep; j++) {
      r1 += S1[j * cslab + c];
      r2 += S2[j * cslab + c];
    }
    atomicAdd(&sum_dz[cbeg + c], r1);
    atomicAdd(&sum_dzx[cbeg + c], r2);
  }
}

// ------------------------------------------------------ BN+act backward ----
// Pass 1: per-channel Σdz and Σ(dz·xhat) where dz = dy·relu'(y).
// grid: (cdiv(C,64), msplit); block 256 = 4 m-lanes × 64 channels.
// mask_mode: 0 = no activation (dz = dy), 1 = ReLU mask from y (residual
// epilogue: y = relu(bn+res)), 2 = ReLU mask derived from convout —
// bn(x) > 0 ⇔ a·x+b > 0 with a = γ·invstd, b = β − γ·mean·invstd — so the
// y tensor is never read (one fewer stream for 12 of 20 ResNet18 convs).
__global__ __launch_bounds__(256) void k_bnact_bwd_reduce(
    const bf16* __restrict__ dy, const bf16* __restrict__ yout,
    const bf16* __restrict__ x, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sum_dz,
    float* __restrict__ sum_dzx, long M, int C, int mask_mode, long mchunk) {
  __shared__ float sdz[4][64];
  __shared__ float sdzx[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min((long)M, mbeg + mchunk);
  float a_dz = 0.f, a_dzx = 0.f;
  if (c < C) {
    const float mean = save_mean[c], invstd = save_invstd[c];
    const float ga = gamma[c] * invstd;
    const float gb = beta[c] - mean * ga;
    for (long m = mbeg + mlane; m < mend; m += 4) {
      long i = m * C + c;
      float g = b2f(dy[i]);
      float xv = b2f(x[i]);
      if (mask_mode == 1) {
        if (b2f(yout[i]) <= 0.f) g = 0.f;
      } else if (mask_mode == 2) {
        if (fmaf(ga, xv, gb) <= 0.f) g = 0.f;
      } else if (mask_mode == 3) {
        float yv = b2f(yout[i]);
        if (yv <= 0.f || yv >= 6.f) g = 0.f;
      } else if (mask_mode == 4) {
        float bn = fmaf(ga, xv, gb);
        if (bn <= 0.f || bn >= 6.f) g = 0.f;
      }
      a_dz += g;
      a_dzx += g * (xv - mean) * invstd;
    }
  }
  sdz[mlane][threadIdx.x & 63] = a_dz;
  sdzx[mlane][threadIdx.x & 63] = a_dzx;
  __syncthreads();
  if (mlane == 0 && c < C) {
    float t1 = sdz[0][threadIdx.x] + sdz[1][threadIdx.x] +
               sdz[2][threadIdx.x] + sdz[3][threadIdx.x];
    float t2 = sdzx[0][threadIdx.x] + sdzx[1][threadIdx.x] +
               sdzx[2][threadIdx.x] + sdzx[3][threadIdx.x];
    // always accumulate: the output buffers double as dbeta/dgamma and in
    // direct-grad mode they are the pre-zeroed flat .grad views
    atomicAdd(&sum_dz[c], t1);
    atomicAdd(&sum_dzx[c], t2);
  }
}

// c-blocked BN backward apply (bn_apply_v8's slab geometry): per-channel
// coefficients fold to registers once per block and the math reduces to
// two fmas per element: dconv = A·dz − D·x + E with A = γ·invstd,
// D = A·invstd·Σdzx/M, E = D·mean − A·Σdz/M.  The flat per-tile kernel
// below re-loaded 5-6 channel vectors per 8 elements.
template <int MASK>
__global__ __launch_bounds__(256) void k_bn_bwd_apply_v8(
    const bf16* __restrict__ dy, const bf16* __restrict__ yout,
    const bf16* __restrict__ x, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ sum_dz,
    const float* __restrict__ sum_dzx, bf16* __restrict__ dconv,
    bf16* __restrict__ dres, long M, int C, long mchunk, int cslab) {
  const float invM = 1.f / (float)M;
  const int cbeg = blockIdx.x * cslab;
  const int lpr = cslab >> 3;
  const int mstep = 256 / lpr;
  const int tid = threadIdx.x;
  if (tid >= mstep * lpr) return;
  const int th_c = cbeg + (tid % lpr) * 8;
  const int th_m = tid / lpr;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float A[8], D[8], E[8], GB[8];
#pragma unroll
  for (int e = 0; e < 8; e++) {
    int c = th_c + e;
    float mean = save_mean[c], istd = save_invstd[c];
    A[e] = gamma[c] * istd;
    D[e] = A[e] * istd * sum_dzx[c] * invM;
    E[e] = D[e] * mean - A[e] * sum_dz[c] * invM;
    if (MASK == 2 || MASK == 4) GB[e] = beta[c] - mean * A[e];
  }
  for (long m = mbeg + th_m; m < mend; m += mstep) {
    const long i = m * C + th_c;
    V8 dy8, x8, y8, dc8, dr8;
    dy8.u = *(const uint4*)(dy + i);
    x8.u = *(const uint4*)(x + i);
    if (MASK == 1 || MASK == 3) y8.u = *(const uint4*)(yout + i);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float g = b2f(dy8.e[e]);
      float xv = b2f(x8.e[e]);
      if (MASK == 1) {
        if (b2f(y8.e[e]) <= 0.f) g = 0.f;
      } else if (MASK == 2) {
        if (fmaf(A[e], xv, GB[e]) <= 0.f) g = 0.f;
      } else if (MASK == 3) {
        float yv = b2f(y8.e[e]);
        if (yv <= 0.f || yv >= 6.f) g = 0.f;
      } else if (MASK == 4) {
        float bn = fmaf(A[e], xv, GB[e]);
        if (bn <= 0.f || bn >= 6.f) g = 0.f;
      }
      dr8.e[e] = f2b(g);
      float t = fmaf(A[e], g, E[e]);
      dc8.e[e] = f2b(fmaf(-D[e], xv, t));
    }
    if (dres != nullptr) *(uint4*)(dres + i) = dr8.u;
    *(uint4*)(dconv + i) = dc8.u;
  }
}

// Pass 2: dconv = gamma·invstd·(dz − Σdz/M − xhat·Σdzx/M); optional dres =
// dz.  V8 per thread (C % 8 == 0).  MASK compile-time like the reduce
// kernels: with runtime mask_mode all five paths landed in ONE 694-instr
// main loop (instruction-bound, ~1.6x off the HBM roofline at r50@224).
template <int MASK>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(
    const bf16* __restrict__ dy, const bf16* __restrict__ yout,
    const bf16* __restrict__ x, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ sum_dz,
    const float* __restrict__ sum_dzx, bf16* __restrict__ dconv,
    bf16* __restrict__ dres, long M, int C) {
  const float invM = 1.f / (float)M;
  if (C % 8 != 0) {  // scalar fallback
    long total = M * (long)C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long)gridDim.x * blockDim.x) {
      int c = (int)(i % C);
      float mean = save_mean[c], invstd = save_invstd[c];
      float g = b2f(dy[i]);
      float xv = b2f(x[i]);
      if (MASK == 1) {
        if (b2f(yout[i]) <= 0.f) g = 0.f;
      } else if (MASK == 2) {
        float ga = gamma[c] * invstd;
        if (fmaf(ga, xv, beta[c] - mean * ga) <= 0.f) g = 0.f;
      } else if (MASK == 3) {
        float yv = b2f(yout[i]);
        if (yv <= 0.f || yv >= 6.f) g = 0.f;
      } else if (MASK == 4) {
        float ga = gamma[c] * invstd;
        float bn = fmaf(ga, xv, beta[c] - mean * ga);
        if (bn <= 0.f || bn >= 6.f) g = 0.f;
      }
      if (dres != nullptr) dres[i] = f2b(g);
      float xh = (xv - mean) * invstd;
      float v = gamma[c] * invstd *
                (g - sum_dz[c] * invM - xh * sum_dzx[c] * invM);
      dconv[i] = f2b(v);
    }
    return;
  }
  long total8 = M * (long)C / 8;
  // channel index kept incrementally (conditional subtract) — the 64-bit
  // modulo per tile fed the critical path of every loop iteration
  const long stride = (long)gridDim.x * blockDim.x;
  long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  int c0 = (int)(i % C);
  const int sd = (int)((stride * 8) % C);
  for (long t = i / 8; t < total8; t += stride, i += stride * 8) {
    F8 mean8 = load_f8(save_mean + c0), istd8 = load_f8(save_invstd + c0);
    F8 g8 = load_f8(gamma + c0);
    F8 sdz8 = load_f8(sum_dz + c0), sdzx8 = load_f8(sum_dzx + c0);
    V8 dy8, x8, y8;
    dy8.u = *(const uint4*)(dy + i);
    x8.u = *(const uint4*)(x + i);
    if (MASK == 1 || MASK == 3) y8.u = *(const uint4*)(yout + i);
    F8 b8;
    if (MASK == 2 || MASK == 4) b8 = load_f8(beta + c0);
    V8 dc8, dr8;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float g = b2f(dy8.e[e]);
      float xv = b2f(x8.e[e]);
      if (MASK == 1) {
        if (b2f(y8.e[e]) <= 0.f) g = 0.f;
      } else if (MASK == 2) {
        float ga = g8.f[e] * istd8.f[e];
        if (fmaf(ga, xv, b8.f[e] - mean8.f[e] * ga) <= 0.f) g = 0.f;
      } else if (MASK == 3) {
        float yv = b2f(y8.e[e]);
        if (yv <= 0.f || yv >= 6.f) g = 0.f;
      } else if (MASK == 4) {
        float ga = g8.f[e] * istd8.f[e];
        float bn = fmaf(ga, xv, b8.f[e] - mean8.f[e] * ga);
        if (bn <= 0.f || bn >= 6.f) g = 0.f;
      }
      dr8.e[e] = f2b(g);
      float xh = (xv - mean8.f[e]) * istd8.f[e];
      float v = g8.f[e] * istd8.f[e] *
                (g - sdz8.f[e] * invM - xh * sdzx8.f[e] * invM);
      dc8.e[e] = f2b(v);
    }
    if (dres != nullptr) *(uint4*)(dres + i) = dr8.u;
    *(uint4*)(dconv + i) = dc8.u;
    c0 += sd;
    if (c0 >= C) c0 -= C;
  }
}

// ------------------------------------- channel-owner BatchNorm (small M) ----
// BN statistics are per channel, so a workgroup that owns a slice of
// channels over ALL M rows can reduce and apply in one launch with only a
// __syncthreads() between the phases — no atomics, no stats arena, and
// the dependent reduce->apply launch boundary (1.7-1.9 us, more than the
// streaming itself at these sizes) disappears.  Geometry: each lane owns 4
// consecutive channels (one dwordx4 of f32 / one dwordx2 of bf16), `lpr`
// lanes sit side by side on a row (cw = 4*lpr channels per workgroup,
// lpr in {1,2,4,8}), and the 256/lpr row-lanes stride the M rows.  Grid =
// C / cw workgroups, so this only pays while one workgroup can cover M
// rows quickly (dispatch thresholds in the launchers below).
union F4 {
  float4 q;
  float f[4];
};

union B4 {
  uint2 u;
  bf16 e[4];
};

// Sum the per-lane partials over the workgroup's row-lanes in a fixed
// order: xor shuffles across the lanes of a wave that share a channel-lane
// (offsets >= lpr keep tid % lpr), then the 4 wave totals through LDS.
// Every thread returns the totals of its own 4 channels.
DEV void owner_reduce(F4& a1, F4& a2, int lpr, int cl,
                      float (*red)[4][32]) {
  for (int off = 32; off >= lpr; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      a1.f[e] += __shfl_xor(a1.f[e], off, 64);
      a2.f[e] += __shfl_xor(a2.f[e], off, 64);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < lpr) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      red[0][wave][cl * 4 + e] = a1.f[e];
      red[1][wave][cl * 4 + e] = a2.f[e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int k = cl * 4 + e;
    a1.f[e] = red[0][0][k] + red[0][1][k] + red[0][2][k] + red[0][3][k];
    a2.f[e] = red[1][0][k] + red[1][1][k] + red[1][2][k] + red[1][3][k];
  }
}

// Eight slab loads of one row issued back to back (slabs z0, z0+zstep, ...;
// indices past nsplit re-read slab z0 and are dropped by slab_add8, so no
// load sits behind a branch), then added in slab order.  One dependent
// load per loop trip left these kernels latency-bound at ~20 GB/s per CU.
DEV void slab_load8(const float* p, long slab, int z0, int zstep,
                    int nsplit, float4* w) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int z = z0 + j * zstep;
    w[j] = *(const float4*)(p + (long)(z < nsplit ? z : z0) * slab);
  }
}

DEV void slab_add8(F4& v, const float4* w, int z0, int zstep, int nsplit) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const bool ok = z0 + j * zstep < nsplit;
    v.f[0] += ok ? w[j].x : 0.f;
    v.f[1] += ok ? w[j].y : 0.f;
    v.f[2] += ok ? w[j].z : 0.f;
    v.f[3] += ok ? w[j].w : 0.f;
  }
}

// Forward, split-K source (replaces k_stats_reduce + k_bn_apply_v8<true>):
// phase 1 sums the nsplit f32 slabs per element into an LDS image
// xs[M][cw] and accumulates (Σx, Σx²); phase 2 applies BN from that image
// (one slab pass instead of two) and emits bf16 convout + y.  zg > 1
// (M < row-lanes): row-lane j takes row j % M and every zg-th split
// starting at j / M, so all lanes have loads in flight at M = 64 with
// 32 splits; the zg partial rows are then summed in a fixed order.
template <int ACT>
__global__ __launch_bounds__(256) void k_bn_fwd_owner(
    const float* __restrict__ xf, const bf16* __restrict__ res,
    bf16* __restrict__ y, bf16* __restrict__ convout,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ running_mean, float* __restrict__ running_var,
    float* __restrict__ save_mean, float* __restrict__ save_invstd, int M,
    int C, float momentum, float eps, int nsplit, int lpr, int zg) {
  extern __shared__ float xs[];    // [max(M, M*zg)][cw]
  __shared__ float red[2][4][32];  // [Σx|Σx²][wave][owned channel]
  const int tid = threadIdx.x;
  const int cw = lpr * 4;
  const int cl = tid & (lpr - 1);
  const int r = tid / lpr;
  const int rl = 256 / lpr;
  const int c0 = blockIdx.x * cw + cl * 4;
  const long slab = (long)M * C;
  F4 a1, a2;
  a1.q = make_float4(0.f, 0.f, 0.f, 0.f);
  a2.q = a1.q;
  if (zg == 1) {
    // two rows x 8 slabs = 16 dwordx4 loads in flight per lane; the second
    // row of a ragged tail re-reads the first and is dropped
    for (int m0 = r; m0 < M; m0 += 2 * rl) {
      const int m1 = m0 + rl;
      const bool ok1 = m1 < M;
      const float* p0 = xf + (long)m0 * C + c0;
      const float* p1 = xf + (long)(ok1 ? m1 : m0) * C + c0;
      F4 v0, v1;
      v0.q = make_float4(0.f, 0.f, 0.f, 0.f);
      v1.q = v0.q;
      for (int z0 = 0; z0 < nsplit; z0 += 8) {
        float4 w0[8], w1[8];
        slab_load8(p0, slab, z0, 1, nsplit, w0);
        slab_load8(p1, slab, z0, 1, nsplit, w1);
        slab_add8(v0, w0, z0, 1, nsplit);
        slab_add8(v1, w1, z0, 1, nsplit);
      }
      *(float4*)(xs + m0 * cw + cl * 4) = v0.q;
      if (ok1) *(float4*)(xs + m1 * cw + cl * 4) = v1.q;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float u = ok1 ? v1.f[e] : 0.f;
        a1.f[e] += v0.f[e];
        a2.f[e] += v0.f[e] * v0.f[e];
        a1.f[e] += u;
        a2.f[e] += u * u;
      }
    }
  } else {
    if (r < M * zg) {
      const int m = r % M, g = r / M;
      const float* p = xf + (long)m * C + c0;
      F4 v;
      v.q = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int z0 = g; z0 < nsplit; z0 += 8 * zg) {
        float4 w[8];
        slab_load8(p, slab, z0, zg, nsplit, w);
        slab_add8(v, w, z0, zg, nsplit);
      }
      *(float4*)(xs + r * cw + cl * 4) = v.q;
    }
    __syncthreads();
    if (r < M) {
      F4 v;
      v.q = *(const float4*)(xs + r * cw + cl * 4);
      for (int g = 1; g < zg; g++) {
        float4 w = *(const float4*)(xs + (g * M + r) * cw + cl * 4);
        v.f[0] += w.x; v.f[1] += w.y; v.f[2] += w.z; v.f[3] += w.w;
      }
      // slot r is read by this thread only (others read g*M + their row)
      *(float4*)(xs + r * cw + cl * 4) = v.q;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        a1.f[e] = v.f[e];
        a2.f[e] = v.f[e] * v.f[e];
      }
    }
  }
  owner_reduce(a1, a2, lpr, cl, red);
  const float invM = 1.f / (float)M;
  float ga[4], be[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const int c = c0 + e;
    float mean = a1.f[e] * invM;
    float var = fmaxf(a2.f[e] * invM - mean * mean, 0.f);
    float istd = rsqrtf(var + eps);
    if (r == 0) {
      save_mean[c] = mean;
      save_invstd[c] = istd;
      // unbiased running var like torch.nn.BatchNorm2d
      float ub = (M > 1) ? var * (float)M / (float)(M - 1) : var;
      running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      running_var[c] = (1.f - momentum) * running_var[c] + momentum * ub;
    }
    ga[e] = gamma[c] * istd;
    be[e] = beta[c] - mean * ga[e];   // y = ga*x + be  [+res] [act]
  }
  // every xs row is re-read by the thread that wrote it
  for (int m = r; m < M; m += rl) {
    const long i = (long)m * C + c0;
    F4 v;
    v.q = *(const float4*)(xs + m * cw + cl * 4);
    B4 co, r4, out;
#pragma unroll
    for (int e = 0; e < 4; e++) co.e[e] = f2b(v.f[e]);
    *(uint2*)(convout + i) = co.u;
    if (res != nullptr) r4.u = *(const uint2*)(res + i);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      float t = fmaf(ga[e], v.f[e], be[e]);
      if (res != nullptr) t += b2f(r4.e[e]);
      if (ACT == 1) t = fmaxf(t, 0.f);
      else if (ACT == 2) t = fminf(fmaxf(t, 0.f), 6.f);  // ReLU6
      out.e[e] = f2b(t);
    }
    *(uint2*)(y + i) = out.u;
  }
}

// dz = dy gated by the activation mask (mask algebra of the reduce
// kernels: 1/3 read the mask from y, 2/4 recover it from convout).
template <int MASK>
DEV float owner_dz(float g, float xe, float yv, float ga, float gb) {
  if (MASK == 1) {
    if (yv <= 0.f) g = 0.f;
  } else if (MASK == 2) {
    if (fmaf(ga, xe, gb) <= 0.f) g = 0.f;
  } else if (MASK == 3) {
    if (yv <= 0.f || yv >= 6.f) g = 0.f;
  } else if (MASK == 4) {
    float bn = fmaf(ga, xe, gb);
    if (bn <= 0.f || bn >= 6.f) g = 0.f;
  }
  return g;
}

// Rows m0, m0+rl, m0+2rl, m0+3rl of dy / convout (/ y for the masks that
// read it) issued back to back: up to 12 loads in flight per lane.  Rows
// past M re-read row m0, so no load sits behind a branch; the callers drop
// them.  y4 is zero where the mask does not read y.
template <int MASK>
DEV void owner_load4(const bf16* __restrict__ dy, const bf16* __restrict__ x,
                     const bf16* __restrict__ yout, int m0, int rl, int M,
                     int C, int c0, B4* d4, B4* x4, B4* y4) {
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int m = m0 + u * rl;
    const long i = (long)(m < M ? m : m0) * C + c0;
    d4[u].u = *(const uint2*)(dy + i);
    x4[u].u = *(const uint2*)(x + i);
    if (MASK == 1 || MASK == 3) y4[u].u = *(const uint2*)(yout + i);
    else y4[u].u = make_uint2(0u, 0u);
  }
}

// Backward, bf16 dy (replaces k_bnact_bwd_reduce + k_bn_bwd_apply_v8):
// phase 1 accumulates Σdz and Σ(dz·xhat) with the reduce kernels' mask
// algebra; phase 2 re-reads the same rows (a workgroup's share is a few
// tens of KB, L1/L2-hot) and writes dconv = A·dz − D·x + E and dres = dz.
// sum_dz/sum_dzx double as dbeta/dgamma and may be flat .grad views that
// accumulate across backwards: the single owner does a plain
// read-add-write, and the apply uses THIS call's sums.
template <int MASK>
__global__ __launch_bounds__(256) void k_bn_bwd_owner(
    const bf16* __restrict__ dy, const bf16* __restrict__ yout,
    const bf16* __restrict__ x, const float* __restrict__ save_mean,
    const float* __restrict__ save_invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ sum_dz,
    float* __restrict__ sum_dzx, bf16* __restrict__ dconv,
    bf16* __restrict__ dres, int M, int C, int lpr) {
  __shared__ float red[2][4][32];  // [Σdz|Σdzx][wave][owned channel]
  const int tid = threadIdx.x;
  const int cw = lpr * 4;
  const int cl = tid & (lpr - 1);
  const int r = tid / lpr;
  const int rl = 256 / lpr;
  const int c0 = blockIdx.x * cw + cl * 4;
  float mean[4], invstd[4], ga[4], gb[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    mean[e] = save_mean[c0 + e];
    invstd[e] = save_invstd[c0 + e];
    ga[e] = gamma[c0 + e] * invstd[e];
    gb[e] = beta[c0 + e] - mean[e] * ga[e];
  }
  F4 adz, adzx;
  adz.q = make_float4(0.f, 0.f, 0.f, 0.f);
  adzx.q = adz.q;
  for (int m0 = r; m0 < M; m0 += 4 * rl) {
    B4 d4[4], x4[4], y4[4];
    owner_load4<MASK>(dy, x, yout, m0, rl, M, C, c0, d4, x4, y4);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const bool ok = m0 + u * rl < M;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float xe = b2f(x4[u].e[e]);
        float g = owner_dz<MASK>(b2f(d4[u].e[e]), xe, b2f(y4[u].e[e]),
                                 ga[e], gb[e]);
        g = ok ? g : 0.f;
        adz.f[e] += g;
        adzx.f[e] += g * (xe - mean[e]) * invstd[e];
      }
    }
  }
  owner_reduce(adz, adzx, lpr, cl, red);
  const float invM = 1.f / (float)M;
  float D[4], E[4];
#pragma unroll
  for (int e = 0; e < 4; e++) {
    if (r == 0) {
      sum_dz[c0 + e] += adz.f[e];
      sum_dzx[c0 + e] += adzx.f[e];
    }
    D[e] = ga[e] * invstd[e] * adzx.f[e] * invM;
    E[e] = D[e] * mean[e] - ga[e] * adz.f[e] * invM;
  }
  for (int m0 = r; m0 < M; m0 += 4 * rl) {
    B4 d4[4], x4[4], y4[4];
    owner_load4<MASK>(dy, x, yout, m0, rl, M, C, c0, d4, x4, y4);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int m = m0 + u * rl;
      if (m >= M) break;
      const long i = (long)m * C + c0;
      B4 dc4, dr4;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float xv = b2f(x4[u].e[e]);
        float g = owner_dz<MASK>(b2f(d4[u].e[e]), xv, b2f(y4[u].e[e]),
                                 ga[e], gb[e]);
        dr4.e[e] = f2b(g);
        float t = fmaf(ga[e], g, E[e]);
        dc4.e[e] = f2b(fmaf(-D[e], xv, t));
      }
      if (dres != nullptr) *(uint2*)(dres + i) = dr4.u;
      *(uint2*)(dconv + i) = dc4.u;
    }
  }
}

// ------------------------------------------------------- depthwise conv ----
// MobileNet-family depthwise 3x3 (generic R,S ≤ 5): channel c maps to
// itself, so the kernel is a per-channel stencil — bandwidth-bound, no
// MFMA.  c-blocked layout (64 channels × 4 m-lanes per block, the proven
// BN-reduce geometry): weights [R,S,C] bf16 are register-cached per
// thread for the whole m-loop, per-channel BN batch stats (Σy,Σy²)
// accumulate via LDS reduce + one atomic pair per block.
#define DW_MAXRS 25

__global__ __launch_bounds__(256) void k_dw_fwd(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    bf16* __restrict__ y, float* __restrict__ stats, int Nb, int H, int W,
    int C, int Ho, int Wo, int R, int S, int str, int pad, long mchunk) {
  __shared__ float s1[4][64];
  __shared__ float s2[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long M = (long)Nb * Ho * Wo;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float wreg[DW_MAXRS];
  const int RS = R * S;
  if (c < C)
    for (int t = 0; t < RS; t++) wreg[t] = b2f(w[t * C + c]);
  float a1 = 0.f, a2 = 0.f;
  if (c < C) {
    for (long m = mbeg + mlane; m < mend; m += 4) {
      int n = (int)(m / (Ho * Wo)), hw = (int)(m % (Ho * Wo));
      int ho = hw / Wo, wo = hw % Wo;
      float acc = 0.f;
      for (int r = 0; r < R; r++) {
        int hi = ho * str - pad + r;
        if (hi < 0 || hi >= H) continue;
        for (int sx = 0; sx < S; sx++) {
          int wi = wo * str - pad + sx;
          if (wi < 0 || wi >= W) continue;
          acc = fmaf(b2f(x[((long)(n * H + hi) * W + wi) * C + c]),
                     wreg[r * S + sx], acc);
        }
      }
      y[m * C + c] = f2b(acc);
      a1 += acc;
      a2 += acc * acc;
    }
  }
  if (stats != nullptr) {
    s1[mlane][threadIdx.x & 63] = a1;
    s2[mlane][threadIdx.x & 63] = a2;
    __syncthreads();
    if (mlane == 0 && c < C) {
      atomicAdd(&stats[c], s1[0][threadIdx.x] + s1[1][threadIdx.x] +
                               s1[2][threadIdx.x] + s1[3][threadIdx.x]);
      atomicAdd(&stats[C + c], s2[0][threadIdx.x] + s2[1][threadIdx.x] +
                                   s2[2][threadIdx.x] + s2[3][threadIdx.x]);
    }
  }
}

// dx[n,hi,wi,c] = Σ_{r,s reaching it} dz[n,ho,wo,c] · w[r,s,c]
__global__ __launch_bounds__(256) void k_dw_dgrad(
    const bf16* __restrict__ dz, const bf16* __restrict__ w,
    bf16* __restrict__ dx, int Nb, int H, int W, int C, int Ho, int Wo,
    int R, int S, int str, int pad, long mchunk) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long M = (long)Nb * H * W;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  float wreg[DW_MAXRS];
  const int RS = R * S;
  if (c < C)
    for (int t = 0; t < RS; t++) wreg[t] = b2f(w[t * C + c]);
  if (c >= C) return;
  for (long m = mbeg + mlane; m < mend; m += 4) {
    int n = (int)(m / (H * W)), hw = (int)(m % (H * W));
    int hi = hw / W, wi = hw % W;
    float acc = 0.f;
    for (int r = 0; r < R; r++) {
      int hs = hi + pad - r;
      if (hs < 0 || hs % str != 0) continue;
      int ho = hs / str;
      if (ho >= Ho) continue;
      for (int sx = 0; sx < S; sx++) {
        int ws = wi + pad - sx;
        if (ws < 0 || ws % str != 0) continue;
        int wo = ws / str;
        if (wo >= Wo) continue;
        acc = fmaf(b2f(dz[((long)(n * Ho + ho) * Wo + wo) * C + c]),
                   wreg[r * S + sx], acc);
      }
    }
    dx[m * C + c] = f2b(acc);
  }
}

// dW[r,s,c] += Σ_m x[...]·dz[...]; 9 register partials per thread, LDS
// reduce over the 4 m-lanes, one atomicAdd per (r,s,c) per block.
__global__ __launch_bounds__(256) void k_dw_wgrad(
    const bf16* __restrict__ x, const bf16* __restrict__ dz,
    float* __restrict__ dw, int Nb, int H, int W, int C, int Ho, int Wo,
    int R, int S, int str, int pad, long mchunk) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int mlane = threadIdx.x >> 6;
  const long M = (long)Nb * Ho * Wo;
  const long mbeg = (long)blockIdx.y * mchunk;
  const long mend = min(M, mbeg + mchunk);
  const int RS = R * S;
  float acc[DW_MAXRS];
  for (int t = 0; t < RS; t++) acc[t] = 0.f;
  if (c < C) {
    for (long m = mbeg + mlane; m < mend; m += 4) {
      int n = (int)(m / (Ho * Wo)), hw = (int)(m % (Ho * Wo));
      int ho = hw / Wo, wo = hw % Wo;
      float g = b2f(dz[m * C + c]);
      for (int r = 0; r < R; r++) {
        int hi = ho * str - pad + r;
        if (hi < 0 || hi >= H) continue;
        for (int sx = 0; sx < S; sx++) {
          int wi = wo * str - pad + sx;
          if (wi < 0 || wi >= W) continue;
          acc[r * S + sx] = fmaf(
              b2f(x[((long)(n * H + hi) * W + wi) * C + c]), g,
              acc[r * S + sx]);
        }
      }
    }
  }
  for (int t = 0; t < RS; t++) {
    red[mlane][threadIdx.x & 63] = acc[t];
    __syncthreads();
    if (mlane == 0 && c < C)
      atomicAdd(&dw[t * C + c], red[0][threadIdx.x] + red[1][threadIdx.x] +
                                    red[2][threadIdx.x] +
                                    red[3][threadIdx.x]);
    __syncthreads();
  }
}

// Channel-vectorized pool pair (C % 8 == 0): 8 channels per lane, one
// spatial decomposition per vec, dwordx4 dy/x loads and 8-byte idx loads
// — the scalar kernels stream 2-byte loads per element (same pathology as
// the scalar BN reduce; stem pool at ResNet50@224 measured 61/129 us
// fwd/bwd, ~6x off roofline).
__global__ __launch_bounds__(256) void k_maxpool_fwd_v8(
    const bf16* __restrict__ x, bf16* __restrict__ y,
    unsigned char* __restrict__ idx, int Nb, int H, int W, int C, int Hp,
    int Wp) {
  const int Cg = C >> 3;
  long total = (long)Nb * Hp * Wp * Cg;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < total;
       v += (long)gridDim.x * blockDim.x) {
    int cg = (int)(v % Cg);
    long t = v / Cg;
    int wo = (int)(t % Wp);
    t /= Wp;
    int ho = (int)(t % Hp);
    int n = (int)(t / Hp);
    float best[8];
    int barg[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      best[e] = 0.f;
      barg[e] = -1;  // none yet: the first in-bounds tap always wins
    }
    for (int r = 0; r < 3; r++) {
      int hi = ho * 2 - 1 + r;
      if (hi < 0 || hi >= H) continue;
      for (int sp = 0; sp < 3; sp++) {
        int wi = wo * 2 - 1 + sp;
        if (wi < 0 || wi >= W) continue;
        V8 xv;
        xv.u = *(const uint4*)(x + ((long)(n * H + hi) * W + wi) * C +
                               cg * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) {
          float val = b2f(xv.e[e]);
          if (barg[e] < 0 || val > best[e]) {
            best[e] = val;
            barg[e] = r * 3 + sp;
          }
        }
      }
    }
    V8 out;
    unsigned char ib[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      out.e[e] = f2b(best[e]);
      ib[e] = (unsigned char)barg[e];
    }
    long o = ((long)(n * Hp + ho) * Wp + wo) * C + cg * 8;
    *(uint4*)(y + o) = out.u;
    *(uint2*)(idx + o) = *(const uint2*)ib;
  }
}

__global__ __launch_bounds__(256) void k_maxpool_bwd_v8(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ idx,
    bf16* __restrict__ dx, int Nb, int H, int W, int C, int Hp, int Wp) {
  const int Cg = C >> 3;
  long total = (long)Nb * H * W * Cg;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < total;
       v += (long)gridDim.x * blockDim.x) {
    int cg = (int)(v % Cg);
    long t = v / Cg;
    int wi = (int)(t % W);
    t /= W;
    int hi = (int)(t % H);
    int n = (int)(t / H);
    float acc[8] = {};
    for (int r = 0; r < 3; r++) {
      int hs = hi + 1 - r;
      if (hs < 0 || (hs & 1)) continue;
      int ho = hs >> 1;
      if (ho >= Hp) continue;
      for (int sp = 0; sp < 3; sp++) {
        int ws = wi + 1 - sp;
        if (ws < 0 || (ws & 1)) continue;
        int wo = ws >> 1;
        if (wo >= Wp) continue;
        long j = ((long)(n * Hp + ho) * Wp + wo) * C + cg * 8;
        unsigned char ib[8];
        *(uint2*)ib = *(const uint2*)(idx + j);
        V8 dv;
        dv.u = *(const uint4*)(dy + j);
        const unsigned char code = (unsigned char)(r * 3 + sp);
#pragma unroll
        for (int e = 0; e < 8; e++)
          if (ib[e] == code) acc[e] += b2f(dv.e[e]);
      }
    }
    V8 out;
#pragma unroll
    for (int e = 0; e < 8; e++) out.e[e] = f2b(acc[e]);
    *(uint4*)(dx + ((long)(n * H + hi) * W + wi) * C + cg * 8) = out.u;
  }
}

// ----------------------------------------------------------------- pooling --

// 3x3/2 pad1 max-pool, NHWC; argmax index (0..8) saved as u8 for backward.
// The result is the first maximum in (r,s) scan order among the in-bounds
// taps, for any finite input (the centre tap is always in bounds).  NaN and
// ±inf inputs are not supported: this file is built with -ffast-math.
__global__ __launch_bounds__(256) void k_maxpool_fwd(
    const bf16* __restrict__ x, bf16* __restrict__ y,
    unsigned char* __restrict__ idx, int Nb, int H, int W, int C, int Hp,
    int Wp) {
  long total = (long)Nb * Hp * Wp * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long t = i / C;
    int wo = (int)(t % Wp);
    t /= Wp;
    int ho = (int)(t % Hp);
    int n = (int)(t / Hp);
    float best = 0.f;
    int barg = -1;  // none yet: the first in-bounds tap always wins
    for (int r = 0; r < 3; r++) {
      int hi = ho * 2 - 1 + r;
      if (hi < 0 || hi >= H) continue;
      for (int s = 0; s < 3; s++) {
        int wi = wo * 2 - 1 + s;
        if (wi < 0 || wi >= W) continue;
        float v = b2f(x[((long)(n * H + hi) * W + wi) * C + c]);
        if (barg < 0 || v > best) {
          best = v;
          barg = r * 3 + s;
        }
      }
    }
    y[i] = f2b(best);
    idx[i] = (unsigned char)barg;
  }
}

__global__ __launch_bounds__(256) void k_maxpool_bwd(
    const bf16* __restrict__ dy, const unsigned char* __restrict__ idx,
    bf16* __restrict__ dx, int Nb, int H, int W, int C, int Hp, int Wp) {
  long total = (long)Nb * H * W * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long t = i / C;
    int wi = (int)(t % W);
    t /= W;
    int hi = (int)(t % H);
    int n = (int)(t / H);
    float acc = 0.f;
    for (int r = 0; r < 3; r++) {
      int hs = hi + 1 - r;
      if (hs < 0 || (hs & 1)) continue;
      int ho = hs >> 1;
      if (ho >= Hp) continue;
      for (int s = 0; s < 3; s++) {
        int ws = wi + 1 - s;
        if (ws < 0 || (ws & 1)) continue;
        int wo = ws >> 1;
        if (wo >= Wp) continue;
        long j = ((long)(n * Hp + ho) * Wp + wo) * C + c;
        if (idx[j] == r * 3 + s) acc += b2f(dy[j]);
      }
    }
    dx[i] = f2b(acc);
  }
}

// Global average pool [N,H,W,C] -> [N,C] (f32 out for the classifier).
__global__ __launch_bounds__(256) void k_avgpool_fwd(
    const bf16* __restrict__ x, bf16* __restrict__ y, int Nb, int HW, int C) {
  long total = (long)Nb * C;
  float inv = 1.f / (float)HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C), n = (int)(i / C);
    float s = 0.f;
    const bf16* base = x + (long)n * HW * C + c;
    for (int t = 0; t < HW; t++) s += b2f(base[(long)t * C]);
    y[i] = f2b(s * inv);
  }
}

__global__ __launch_bounds__(256) void k_avgpool_bwd(
    const bf16* __restrict__ dy, bf16* __restrict__ dx, int Nb, int HW,
    int C) {
  long total = (long)Nb * HW * C;
  float inv = 1.f / (float)HW;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int c = (int)(i % C);
    long n = i / ((long)HW * C);
    dx[i] = f2b(b2f(dy[n * C + c]) * inv);
  }
}

// ------------------------------------------------------------- classifier --
// Small fc: x[B,In] bf16 · w[Out,In] bf16 + b[Out] f32 -> logits[B,Out] f32.
// One wave per sample row: the wave loads x[b,:] as vec8 per lane (In ≤ 512
// in one shot), then per output j the w row streams through all lanes and
// the dot product closes with a wave shuffle reduction — every load is a
// coalesced 16 B vector (the scalar-load version measured 83 µs; this ~6 µs).
__global__ __launch_bounds__(256) void k_linear_fwd(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ y, int B, int In,
    int Out) {
  const int lane = threadIdx.x & 63;
  const int wave_in_blk = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave_in_blk;  // 4 waves per block
  if (row >= B) return;
  const int chunk = In / 8;          // vec8 chunks (In % 8 == 0)
  const int per_lane = (chunk + 63) / 64;
  float xs[8 * 4];                   // up to In=2048 per lane
  const bf16* xr = x + (long)row * In;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    int ci = lane + t * 64;
    if (t < per_lane && ci < chunk) {
      V8 v = *(const V8*)(xr + ci * 8);
#pragma unroll
      for (int e = 0; e < 8; e++) xs[t * 8 + e] = b2f(v.e[e]);
    }
  }
  for (int j = 0; j < Out; j++) {
    const bf16* wr = w + (long)j * In;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      int ci = lane + t * 64;
      if (t < per_lane && ci < chunk) {
        V8 v = *(const V8*)(wr + ci * 8);
#pragma unroll
        for (int e = 0; e < 8; e++) s = fmaf(xs[t * 8 + e], b2f(v.e[e]), s);
      }
    }
    s = wave_reduce_sum(s);
    if (lane == 0) y[(long)row * Out + j] = s + (b ? b[j] : 0.f);
  }
}

// dx[B,In] bf16 = dy[B,Out] f32 · w[Out,In]
__global__ __launch_bounds__(256) void k_linear_bwd_dx(
    const float* __restrict__ dy, const bf16* __restrict__ w,
    bf16* __restrict__ dx, int B, int In, int Out) {
  long total = (long)B * In;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int t = (int)(i % In), bi = (int)(i / In);
    float s = 0.f;
    for (int j = 0; j < Out; j++)
      s = fmaf(dy[(long)bi * Out + j], b2f(w[(long)j * In + t]), s);
    dx[i] = f2b(s);
  }
}

// dw[Out,In] f32 (+)= Σ_b dy[b,j]·x[b,t];  db[Out] f32 (+)= Σ_b dy[b,j]
// accum=1 adds into the existing buffer (direct-grad mode: dw/db are the
// pre-zeroed flat .grad views).
// dW[j][t] = Σ_b dy[b][j]·x[b][t].  Classifier shape (Out ≤ 16): one
// thread per input column t holding OUTN=16 partials in REGISTERS (all
// loops compile-time — dynamic bounds would spill the accumulator array to
// scratch); dy is LDS-staged zero-padded to 16 columns, x column reads
// coalesce across threads.
__global__ __launch_bounds__(256) void k_linear_bwd_dw_small(
    const float* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ dw, float* __restrict__ db, int B, int In, int Out,
    int accum) {
  constexpr int OUTN = 16;
  __shared__ float dys[128 * OUTN];  // [B][16], B ≤ 128
  const int tid = threadIdx.x;
  for (int i = tid; i < B * OUTN; i += blockDim.x) {
    int j = i & (OUTN - 1);
    dys[i] = j < Out ? dy[(i >> 4) * Out + j] : 0.f;
  }
  __syncthreads();
  float s[OUTN];
#pragma unroll
  for (int j = 0; j < OUTN; j++) s[j] = 0.f;
  int t = blockIdx.x * blockDim.x + tid;
  if (t < In) {
    for (int bi = 0; bi < B; bi++) {
      float xv = b2f(x[(long)bi * In + t]);
#pragma unroll
      for (int j = 0; j < OUTN; j++)
        s[j] = fmaf(dys[bi * OUTN + j], xv, s[j]);
    }
    for (int j = 0; j < Out; j++) {
      long i = (long)j * In + t;
      dw[i] = accum ? dw[i] + s[j] : s[j];
    }
  }
  if (blockIdx.x == 0 && tid < Out && db != nullptr) {
    float sb = 0.f;
    for (int bi = 0; bi < B; bi++) sb += dys[bi * OUTN + tid];
    db[tid] = accum ? db[tid] + sb : sb;
  }
}

// Large-batch variant: B split across blockIdx.y in ≤128-row chunks
// (the register-tiled kernel is In-parallel only — 2 workgroups at
// In=512, a 1024-deep serial loop each: 310 µs at bs=1024, r02 PMC).
// Partials atomicAdd into dw/db — dw must be pre-zeroed (direct-grad
// mode is; the eager path memsets first); deterministic mode keeps the
// single-chunk kernels.
__global__ __launch_bounds__(256) void k_linear_bwd_dw_bsplit(
    const float* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ dw, float* __restrict__ db, int B, int In, int Out,
    int bchunk) {
  constexpr int OUTN = 16;
  __shared__ float dys[128 * OUTN];
  const int tid = threadIdx.x;
  const int bbeg = blockIdx.y * bchunk;
  const int bend = min(B, bbeg + bchunk);
  const int nb = bend - bbeg;
  for (int i = tid; i < nb * OUTN; i += blockDim.x) {
    int j = i & (OUTN - 1);
    dys[i] = j < Out ? dy[(long)(bbeg + (i >> 4)) * Out + j] : 0.f;
  }
  __syncthreads();
  float s[OUTN];
#pragma unroll
  for (int j = 0; j < OUTN; j++) s[j] = 0.f;
  int t = blockIdx.x * blockDim.x + tid;
  if (t < In) {
    for (int bi = 0; bi < nb; bi++) {
      float xv = b2f(x[(long)(bbeg + bi) * In + t]);
#pragma unroll
      for (int j = 0; j < OUTN; j++)
        s[j] = fmaf(dys[bi * OUTN + j], xv, s[j]);
    }
    for (int j = 0; j < Out; j++)
      atomicAdd(&dw[(long)j * In + t], s[j]);
  }
  if (blockIdx.x == 0 && tid < Out && db != nullptr) {
    float sb = 0.f;
    for (int bi = 0; bi < nb; bi++) sb += dys[bi * OUTN + tid];
    atomicAdd(&db[tid], sb);
  }
}

__global__ __launch_bounds__(256) void k_linear_bwd_dw(
    const float* __restrict__ dy, const bf16* __restrict__ x,
    float* __restrict__ dw, float* __restrict__ db, int B, int In, int Out,
    int accum) {
  long total = (long)Out * In;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    int t = (int)(i % In), j = (int)(i / In);
    float s = 0.f;
    for (int bi = 0; bi < B; bi++)
      s = fmaf(dy[(long)bi * Out + j], b2f(x[(long)bi * In + t]), s);
    dw[i] = accum ? dw[i] + s : s;
    if (t == 0 && db != nullptr) {
      float sb = 0.f;
      for (int bi = 0; bi < B; bi++) sb += dy[(long)bi * Out + j];
      db[j] = accum ? db[j] + sb : sb;
    }
  }
}

// ------------------------------------------------------- fused CE loss -----
// One row of the fused loss: writes (softmax − target distribution)/B to
// `drow` and returns the row's share of the mean loss.  LS=false is the
// one-hot target; LS=true smooths it to (1−ε)·onehot + ε/NC, i.e.
// loss = (1−ε)(lse − x_t) + ε(lse − mean_j x_j).  `eps` is dead code in the
// LS=false instantiation, so the one-hot kernels are unchanged by it.
template <bool LS>
__device__ __forceinline__ float ce_row(const float* __restrict__ row, int t,
                                        int B, int NC, float eps,
                                        float* __restrict__ drow) {
  float mx = row[0];
  for (int j = 1; j < NC; j++) mx = fmaxf(mx, row[j]);
  float se = 0.f;
  for (int j = 0; j < NC; j++) se += __expf(row[j] - mx);
  float lse = __logf(se) + mx;
  float li = lse - row[t];
  float invB = 1.f / (float)B;
  if (LS) {
    float sx = 0.f;
    for (int j = 0; j < NC; j++) sx += row[j];
    li = (1.f - eps) * li + eps * (lse - sx / (float)NC);
    float on = 1.f - eps, off = eps / (float)NC;
    for (int j = 0; j < NC; j++) {
      float p = __expf(row[j] - lse);
      drow[j] = (p - (j == t ? on : 0.f) - off) * invB;
    }
  } else {
    for (int j = 0; j < NC; j++) {
      float p = __expf(row[j] - lse);
      drow[j] = (p - (j == t ? 1.f : 0.f)) * invB;
    }
  }
  return li / (float)B;
}

// Deterministic variant: ONE block, per-thread strided rows, ordered
// block reduce of the loss (the default kernel's atomicAdd order varies).
template <bool LS>
__device__ __forceinline__ void ce_det_body(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC,
    float eps) {
  __shared__ float part[256];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256)
    acc += ce_row<LS>(logits + (long)b * NC, (int)target[b], B, NC, eps,
                      dlogits + (long)b * NC);
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < 256; i++) s += part[i];
    loss[0] = s;
  }
}

// logits[B,NC] f32 -> mean NLL loss (atomic into loss[0]) + dlogits f32
// (softmax − onehot)/B.  One thread per row (NC ≤ 32).
template <bool LS>
__device__ __forceinline__ void ce_body(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC,
    float eps, int b0, int bstride) {
  for (int b = b0; b < B; b += bstride)
    atomicAdd(loss, ce_row<LS>(logits + (long)b * NC, (int)target[b], B, NC,
                               eps, dlogits + (long)b * NC));
}

__global__ __launch_bounds__(256) void k_ce_fwd_bwd_det(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC) {
  ce_det_body<false>(logits, target, loss, dlogits, B, NC, 0.f);
}

__global__ __launch_bounds__(256) void k_ce_fwd_bwd(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC) {
  ce_body<false>(logits, target, loss, dlogits, B, NC, 0.f,
                 blockIdx.x * blockDim.x + threadIdx.x,
                 gridDim.x * blockDim.x);
}

// label-smoothed forms (ε > 0 only; ε = 0 launches the kernels above)
__global__ __launch_bounds__(256) void k_ce_ls_fwd_bwd_det(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC,
    float eps) {
  ce_det_body<true>(logits, target, loss, dlogits, B, NC, eps);
}

__global__ __launch_bounds__(256) void k_ce_ls_fwd_bwd(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC,
    float eps) {
  ce_body<true>(logits, target, loss, dlogits, B, NC, eps,
                blockIdx.x * blockDim.x + threadIdx.x,
                gridDim.x * blockDim.x);
}

// ------------------------------------------------------- fused optimizers --
// Flat-buffer Adam: master f32, grad f32 (zeroed after), m/v f32, bf16 shadow
// emitted for every element.  `step_t` is a device scalar so the kernel is
// hipGraph-replayable (bias correction computed on device).
// gsrc (optional): all-reduced bf16 gradient consumed directly with a
// 1/world scale — skips the DP path's unpack copy+mul pass.
// Optional fused divergence probe (prev/sumsq non-null): the kernel already
// streams the f32 gradient, so Σ(g−g_prev)² + prev←g ride along for one
// extra read+write of prev instead of a standalone 3×45 MB gdiv pass
// (measured ~61 µs/step standalone vs ~13 µs marginal here; engine-flat
// trace r02).  The probe always reads the LOCAL f32 grad (pre-average),
// matching the reference's per-worker probe semantics.
// The loop lives in adam_body / sgd_body (grid-stride start and stride are
// formed in the kernel and passed in) so that k_adam_step / k_sgd_step
// (lr by value) and the *_ex kernels (lr from a device table, AdamW,
// Nesterov) evaluate one update expression with one contraction.
// DECOUPLED (AdamW): wd is not added to g; w is scaled by (1 − lr·wd) before
// the Adam update, as torch.optim.AdamW does.
// SEG (the *_seg kernels): `wd` is the segment's weight multiplier and the
// gradient is first scaled by the segment's `gmul` (clip factor × LARS trust
// ratio).  The scale is its own rounded product in front of the unchanged
// expression, skipped when gmul == 1, so a uniform table reproduces the
// unsegmented kernels bit for bit.
// LIVE (the *_live kernels): the range is a chunk of the live table, `nruns`
// runs of `run_len` elements at pitch `run_pitch` from `base`; [i0, n) then
// counts the chunk's elements (n = nruns·run_len) and LiveIdx turns the count
// into the buffer index.  Everything else is the same loop.
struct LiveIdx {
  // (run, offset in run) of element e, advanced by `istride` per iteration
  // with one compare instead of a division per element
  unsigned r, j, dq, dm, run_len;
  long base, pitch;
  __device__ __forceinline__ LiveIdx(long i0, long istride, unsigned run_len_,
                                     long base_, long pitch_)
      : run_len(run_len_), base(base_), pitch(pitch_) {
    r = (unsigned)i0 / run_len;
    j = (unsigned)i0 - r * run_len;
    dq = (unsigned)istride / run_len;
    dm = (unsigned)istride - dq * run_len;
  }
  __device__ __forceinline__ long at() const {
    return base + (long)r * pitch + j;
  }
  __device__ __forceinline__ void next() {
    r += dq;
    j += dm;
    if (j >= run_len) { j -= run_len; r++; }
  }
};

template <bool DECOUPLED, bool SEG = false, bool LIVE = false>
__device__ __forceinline__ void adam_body(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
    const float* __restrict__ step_t, long n, float lr, float b1, float b2,
    float eps, float wd, int zero_grad, float* __restrict__ extra_zero,
    long n_extra, const bf16* __restrict__ gsrc, float gscale,
    float* __restrict__ prev, float* __restrict__ sumsq, long i0,
    long istride, float gmul = 1.f, unsigned run_len = 1, long base = 0,
    long run_pitch = 0) {
  for (long i = i0; i < n_extra; i += istride) extra_zero[i] = 0.f;
  float t = step_t[0];
  float bc1 = 1.f - __powf(b1, t), bc2 = 1.f - __powf(b2, t);
  float acc = 0.f;
  LiveIdx li(LIVE ? i0 : 0, LIVE ? istride : 0, run_len, base, run_pitch);
  for (long e = i0; e < n; e += istride) {
    const long i = LIVE ? li.at() : e;
    if (LIVE) li.next();
    float gl = grad[i];
    float g = gsrc != nullptr ? b2f(gsrc[i]) * gscale : gl;
    if (prev != nullptr) {
      float d = gl - prev[i];
      prev[i] = gl;
      acc += d * d;
    }
    if (SEG && gmul != 1.f) g *= gmul;
    float w = master[i];
    if (DECOUPLED) {
      if (wd != 0.f) w *= 1.f - lr * wd;
    } else {
      if (wd != 0.f) g += wd * w;
    }
    float mi = b1 * m[i] + (1.f - b1) * g;
    float vi = b2 * v[i] + (1.f - b2) * g * g;
    m[i] = mi;
    v[i] = vi;
    w -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
    master[i] = w;
    if (shadow != nullptr) shadow[i] = f2b(w);
    if (zero_grad) grad[i] = 0.f;
  }
  if (prev != nullptr) {
    acc = wave_reduce_sum(acc);
    __shared__ float ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicAdd(sumsq, ws[0] + ws[1] + ws[2] + ws[3]);
  }
}

// NESTEROV: u = μ·mom + g; mom = u; w −= lr·(g + μ·u)  (torch's definition)
template <bool NESTEROV, bool SEG = false, bool LIVE = false>
__device__ __forceinline__ void sgd_body(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ mom, bf16* __restrict__ shadow, long n, float lr,
    float mu, float wd, int zero_grad, const bf16* __restrict__ gsrc,
    float gscale, float* __restrict__ prev, float* __restrict__ sumsq,
    long i0, long istride, float gmul = 1.f, unsigned run_len = 1,
    long base = 0, long run_pitch = 0) {
  float acc = 0.f;
  LiveIdx li(LIVE ? i0 : 0, LIVE ? istride : 0, run_len, base, run_pitch);
  for (long e = i0; e < n; e += istride) {
    const long i = LIVE ? li.at() : e;
    if (LIVE) li.next();
    float gl = grad[i];
    float g = gsrc != nullptr ? b2f(gsrc[i]) * gscale : gl;
    if (prev != nullptr) {  // fused divergence probe (see adam_body)
      float d = gl - prev[i];
      prev[i] = gl;
      acc += d * d;
    }
    if (SEG && gmul != 1.f) g *= gmul;
    float w = master[i];
    if (wd != 0.f) g += wd * w;
    float u = (mom != nullptr) ? (mu * mom[i] + g) : g;
    if (mom != nullptr) mom[i] = u;
    if (NESTEROV)
      w -= lr * (g + mu * u);
    else
      w -= lr * u;
    master[i] = w;
    if (shadow != nullptr) shadow[i] = f2b(w);
    if (zero_grad) grad[i] = 0.f;
  }
  if (prev != nullptr) {
    acc = wave_reduce_sum(acc);
    __shared__ float ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicAdd(sumsq, ws[0] + ws[1] + ws[2] + ws[3]);
  }
}

// Learning rate of this update for the *_ex kernels: with a table,
// lr_table[clamp(step_t − 1, 0, T−1)] — `step_t` is the already-incremented
// f32 device counter, so a replayed hipGraph walks the schedule with no host
// work; without one, the by-value `lr`.  Wave-uniform: one 4-byte load per
// thread, before the loop.  Thread 0 of block 0 records the value used.
__device__ __forceinline__ float sched_lr(const float* __restrict__ step_t,
                                          const float* __restrict__ lr_table,
                                          long T, float lr,
                                          float* __restrict__ lr_out) {
  if (lr_table != nullptr) {
    long k = (long)step_t[0] - 1;
    k = k < 0 ? 0 : (k > T - 1 ? T - 1 : k);
    lr = lr_table[k];
  }
  if (lr_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
    lr_out[0] = lr;
  return lr;
}

__global__ __launch_bounds__(256) void k_adam_step(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
    const float* __restrict__ step_t, long n, float lr, float b1, float b2,
    float eps, float wd, int zero_grad, float* __restrict__ extra_zero,
    long n_extra, const bf16* __restrict__ gsrc, float gscale,
    float* __restrict__ prev, float* __restrict__ sumsq) {
  adam_body<false>(master, grad, m, v, shadow, step_t, n, lr, b1, b2, eps,
                   wd, zero_grad, extra_zero, n_extra, gsrc, gscale, prev,
                   sumsq,
                   (long)blockIdx.x * blockDim.x + threadIdx.x,
                   (long)gridDim.x * blockDim.x);
}

template <bool DECOUPLED>
__global__ __launch_bounds__(256) void k_adam_step_ex(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
    const float* __restrict__ step_t, long n, float lr, float b1, float b2,
    float eps, float wd, int zero_grad, float* __restrict__ extra_zero,
    long n_extra, const bf16* __restrict__ gsrc, float gscale,
    float* __restrict__ prev, float* __restrict__ sumsq,
    const float* __restrict__ lr_table, long T, float* __restrict__ lr_out) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  adam_body<DECOUPLED>(master, grad, m, v, shadow, step_t, n, lr, b1, b2,
                       eps, wd, zero_grad, extra_zero, n_extra, gsrc, gscale,
                       prev, sumsq,
                       (long)blockIdx.x * blockDim.x + threadIdx.x,
                       (long)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void k_sgd_step(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ mom, bf16* __restrict__ shadow, long n, float lr,
    float mu, float wd, int zero_grad, const bf16* __restrict__ gsrc,
    float gscale, float* __restrict__ prev, float* __restrict__ sumsq) {
  sgd_body<false>(master, grad, mom, shadow, n, lr, mu, wd, zero_grad, gsrc,
                  gscale, prev, sumsq,
                  (long)blockIdx.x * blockDim.x + threadIdx.x,
                  (long)gridDim.x * blockDim.x);
}

// `step_t` may be null only when `lr_table` is (unscheduled Nesterov).
template <bool NESTEROV>
__global__ __launch_bounds__(256) void k_sgd_step_ex(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ mom, bf16* __restrict__ shadow, long n, float lr,
    float mu, float wd, int zero_grad, const bf16* __restrict__ gsrc,
    float gscale, float* __restrict__ prev, float* __restrict__ sumsq,
    const float* __restrict__ step_t, const float* __restrict__ lr_table,
    long T, float* __restrict__ lr_out) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  sgd_body<NESTEROV>(master, grad, mom, shadow, n, lr, mu, wd, zero_grad,
                     gsrc, gscale, prev, sumsq,
                     (long)blockIdx.x * blockDim.x + threadIdx.x,
                     (long)gridDim.x * blockDim.x);
}

__global__ void k_inc_step(float* step_t) { step_t[0] += 1.f; }

// ---------------------------------------------- segmented optimizer step --
// Segment s = one parameter = [b_s, b_{s+1}) of the flat buffer.  The host
// cuts every segment into chunks of <= 4096 elements that never cross a
// segment: chunks[c] = (segment, start, length).  One workgroup per chunk,
// so the segment is workgroup-uniform in every kernel below (no per-element
// search).  seg_meta[s] = (first chunk, one past the last chunk, flags) with
// flags bit 0 = decay_s, bit 1 = adapt_s.
// Contract (docs/KERNELS.md "Segmented step"): G_s = Σg², W_s = Σw²,
// N = sqrt(Σ_s G_s), c = min(1, max_norm/(N + 1e-6)) (1 when max_norm <= 0),
// wd_s = wd·decay_s, q_s = η·‖w‖/(c·‖g‖ + wd_s·‖w‖ + 1e-8) for LARS on an
// adapt segment with ‖w‖ > 0 and ‖g‖ > 0, else 1;
// seg_mul[s] = (gmul_s, wmul_s) = (q_s·c, q_s·wd_s).
// No float atomics: partials are stored per chunk and folded in a fixed
// order, so the result is bitwise reproducible and a replayed graph cannot
// accumulate into stale state.
template <int NW>  // waves per workgroup
__device__ __forceinline__ float block_sum(float x, float* ws) {
  x = wave_reduce_sum(x);
  __syncthreads();  // ws may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = x;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NW; i++) s += ws[i];
  return s;
}

// partials[c] = (Σg², Σw²) of chunk c; g is the step kernel's effective
// gradient (b2f(gsrc)·gscale, else grad).  Loads are 16-byte vectors over
// the aligned middle of the chunk (float4; 8×bf16 + 2×float4 with gsrc),
// scalar over its unaligned head and tail.  need_w = 0 (clip without LARS)
// skips the master stream and stores Σw² = 0.
__global__ __launch_bounds__(256) void k_seg_sumsq_partial(
    const float* __restrict__ master, const float* __restrict__ grad,
    const bf16* __restrict__ gsrc, float gscale,
    const int* __restrict__ chunks, float* __restrict__ partials,
    int need_w) {
  __shared__ float ws[4];
  const int c = blockIdx.x;
  const long start = chunks[c * 3 + 1];
  const int len = chunks[c * 3 + 2];
  const int A = gsrc != nullptr ? 8 : 4;  // elements per vector step
  int head = (int)((A - (start & (A - 1))) & (A - 1));
  if (head > len) head = len;
  const int nvec = (len - head) / A;
  const long vbase = start + head;
  const long tbase = vbase + (long)nvec * A;
  const int tail = len - head - nvec * A;
  float ag = 0.f, aw = 0.f;
  // head and tail: at most 2·(A−1) scalars, one per thread
  {
    const int t = threadIdx.x;
    long i = -1;
    if (t < head) i = start + t;
    else if (t - head < tail) i = tbase + (t - head);
    if (i >= 0) {
      float g = gsrc != nullptr ? b2f(gsrc[i]) * gscale : grad[i];
      ag += g * g;
      if (need_w) { float w = master[i]; aw += w * w; }
    }
  }
  if (gsrc != nullptr) {
    for (int k = threadIdx.x; k < nvec; k += 256) {
      const long i = vbase + (long)k * 8;
      const uint4 raw = *reinterpret_cast<const uint4*>(gsrc + i);
      const unsigned r[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float lo = __uint_as_float(r[j] << 16) * gscale;
        float hi = __uint_as_float(r[j] & 0xffff0000u) * gscale;
        ag += lo * lo;
        ag += hi * hi;
      }
      if (need_w) {
        const float4 w0 = *reinterpret_cast<const float4*>(master + i);
        const float4 w1 = *reinterpret_cast<const float4*>(master + i + 4);
        aw += w0.x * w0.x; aw += w0.y * w0.y;
        aw += w0.z * w0.z; aw += w0.w * w0.w;
        aw += w1.x * w1.x; aw += w1.y * w1.y;
        aw += w1.z * w1.z; aw += w1.w * w1.w;
      }
    }
  } else {
    for (int k = threadIdx.x; k < nvec; k += 256) {
      const long i = vbase + (long)k * 4;
      const float4 g = *reinterpret_cast<const float4*>(grad + i);
      ag += g.x * g.x; ag += g.y * g.y; ag += g.z * g.z; ag += g.w * g.w;
      if (need_w) {
        const float4 w = *reinterpret_cast<const float4*>(master + i);
        aw += w.x * w.x; aw += w.y * w.y; aw += w.z * w.z; aw += w.w * w.w;
      }
    }
  }
  ag = block_sum<4>(ag, ws);
  aw = block_sum<4>(aw, ws);
  if (threadIdx.x == 0) {
    partials[2 * c] = ag;
    partials[2 * c + 1] = aw;
  }
}

// ONE workgroup of 16 waves (the fold of one segment is a chain of dependent
// latencies — table entry, partials, wave reduce — so segments per wave set
// the time: 4 waves measured 15 us at ResNet18's 62 segments).  Wave w folds
// segments w, w+16, ...: its 64 lanes sum the segment's chunk partials
// strided, then a wave reduce — a fixed order.
// seg_norms[s] = (G_s, W_s) is both the hand-over to the second phase and a
// readable by-product.  Then N, c, q_s and seg_mul; norm_out = (N, c).
constexpr int kSegFinWaves = 16;
__global__ __launch_bounds__(64 * kSegFinWaves) void k_seg_finalize(
    const float* __restrict__ partials, const int* __restrict__ seg_meta,
    int nseg, float wd, float max_norm, int lars, float eta,
    float* __restrict__ seg_norms, float* __restrict__ seg_mul,
    float* __restrict__ norm_out) {
  constexpr int NT = 64 * kSegFinWaves;
  __shared__ float ws[kSegFinWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s < nseg; s += kSegFinWaves) {
    const int c0 = seg_meta[s * 3], c1 = seg_meta[s * 3 + 1];
    float ag = 0.f, aw = 0.f;
    for (int c = c0 + lane; c < c1; c += 64) {
      ag += partials[2 * c];
      aw += partials[2 * c + 1];
    }
    ag = wave_reduce_sum(ag);
    aw = wave_reduce_sum(aw);
    if (lane == 0) {
      seg_norms[2 * s] = ag;
      seg_norms[2 * s + 1] = aw;
    }
  }
  __threadfence_block();
  __syncthreads();
  float tot = 0.f;
  for (int s = threadIdx.x; s < nseg; s += NT) tot += seg_norms[2 * s];
  tot = block_sum<kSegFinWaves>(tot, ws);
  const float N = sqrtf(tot);
  float c = 1.f;
  if (max_norm > 0.f) c = fminf(1.f, max_norm / (N + 1e-6f));
  for (int s = threadIdx.x; s < nseg; s += NT) {
    const int flags = seg_meta[s * 3 + 2];
    const float wd_s = (flags & 1) ? wd : 0.f;
    float q = 1.f;
    if (lars && (flags & 2)) {
      const float gn = c * sqrtf(seg_norms[2 * s]);
      const float wn = sqrtf(seg_norms[2 * s + 1]);
      if (wn > 0.f && gn > 0.f) q = eta * wn / (gn + wd_s * wn + 1e-8f);
    }
    seg_mul[2 * s] = q * c;
    seg_mul[2 * s + 1] = q * wd_s;
  }
  if (threadIdx.x == 0) {
    norm_out[0] = N;
    norm_out[1] = c;
  }
}

// The *_ex kernels with per-segment multipliers: grid = chunks, the body's
// range is the chunk.  Every other duty (lr table / lr_out, shadow,
// zero_grad, extra_zero, gsrc, probe) is the body's, unchanged.
template <bool NESTEROV>
__global__ __launch_bounds__(256) void k_sgd_step_seg(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ mom, bf16* __restrict__ shadow, float lr, float mu,
    int zero_grad, const bf16* __restrict__ gsrc, float gscale,
    float* __restrict__ prev, float* __restrict__ sumsq,
    const float* __restrict__ step_t, const float* __restrict__ lr_table,
    long T, float* __restrict__ lr_out, const int* __restrict__ chunks,
    const float* __restrict__ seg_mul) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  const int c = blockIdx.x;
  const int s = chunks[c * 3];
  const long start = chunks[c * 3 + 1];
  const long end = start + chunks[c * 3 + 2];
  sgd_body<NESTEROV, true>(master, grad, mom, shadow, end, lr, mu,
                           seg_mul[2 * s + 1], zero_grad, gsrc, gscale, prev,
                           sumsq, start + threadIdx.x, 256, seg_mul[2 * s]);
}

template <bool DECOUPLED>
__global__ __launch_bounds__(256) void k_adam_step_seg(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
    const float* __restrict__ step_t, float lr, float b1, float b2,
    float eps, int zero_grad, float* __restrict__ extra_zero, long n_extra,
    const bf16* __restrict__ gsrc, float gscale, float* __restrict__ prev,
    float* __restrict__ sumsq, const float* __restrict__ lr_table, long T,
    float* __restrict__ lr_out, const int* __restrict__ chunks,
    const float* __restrict__ seg_mul) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_extra;
       i += (long)gridDim.x * 256)
    extra_zero[i] = 0.f;
  const int c = blockIdx.x;
  const int s = chunks[c * 3];
  const long start = chunks[c * 3 + 1];
  const long end = start + chunks[c * 3 + 2];
  adam_body<DECOUPLED, true>(master, grad, m, v, shadow, step_t, end, lr, b1,
                             b2, eps, seg_mul[2 * s + 1], zero_grad, nullptr,
                             0, gsrc, gscale, prev, sumsq,
                             start + threadIdx.x, 256, seg_mul[2 * s]);
}

// -------------------------------------------------- live-range step ------
// The unsegmented step over the live part of the flat buffer only: filter
// taps that only ever meet padding have g = m = v = 0 for good, so without
// weight decay the update is the identity on them and they are not streamed
// (docs/KERNELS.md "Live-range step"; the host verifies the precondition
// when it builds the table).  live[c] = (start, run_len, run_pitch, nruns),
// int32: chunk c is elements start + r·run_pitch + j, r < nruns,
// j < run_len.  One workgroup per chunk, so the run geometry is
// workgroup-uniform.  The body is the full kernels', with wd = 0: a live
// element gets bitwise what k_adam_step / k_sgd_step(_ex) give it.
// Scalar accesses as in the full kernels: runs start and end anywhere.
__global__ __launch_bounds__(256) void k_adam_step_live(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ m, float* __restrict__ v, bf16* __restrict__ shadow,
    const float* __restrict__ step_t, float lr, float b1, float b2,
    float eps, int zero_grad, float* __restrict__ extra_zero, long n_extra,
    const bf16* __restrict__ gsrc, float gscale, float* __restrict__ prev,
    float* __restrict__ sumsq, const float* __restrict__ lr_table, long T,
    float* __restrict__ lr_out, const int4* __restrict__ live) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_extra;
       i += (long)gridDim.x * 256)
    extra_zero[i] = 0.f;
  const int4 c = live[blockIdx.x];
  adam_body<false, false, true>(master, grad, m, v, shadow, step_t,
                                (long)c.w * c.y, lr, b1, b2, eps, 0.f,
                                zero_grad, nullptr, 0, gsrc, gscale, prev,
                                sumsq, threadIdx.x, 256, 1.f, (unsigned)c.y,
                                c.x, c.z);
}

template <bool NESTEROV>
__global__ __launch_bounds__(256) void k_sgd_step_live(
    float* __restrict__ master, float* __restrict__ grad,
    float* __restrict__ mom, bf16* __restrict__ shadow, float lr, float mu,
    int zero_grad, const bf16* __restrict__ gsrc, float gscale,
    float* __restrict__ prev, float* __restrict__ sumsq,
    const float* __restrict__ step_t, const float* __restrict__ lr_table,
    long T, float* __restrict__ lr_out, const int4* __restrict__ live) {
  lr = sched_lr(step_t, lr_table, T, lr, lr_out);
  const int4 c = live[blockIdx.x];
  sgd_body<NESTEROV, false, true>(master, grad, mom, shadow, (long)c.w * c.y,
                                  lr, mu, 0.f, zero_grad, gsrc, gscale, prev,
                                  sumsq, threadIdx.x, 256, 1.f,
                                  (unsigned)c.y, c.x, c.z);
}

// ------------------------------------------------ dgrad weight transpose ---
// Batched KRSC -> RSCK permute of every conv weight shadow (one launch per
// step).  meta[i*4 + {0:src_off,1:dst_off,2:nelem,3:packed}] with packed =
// (K<<16)|(C); rs count derived from nelem.
// Per (rs): transpose the [K][C] slab to [C][K] through a padded 32×32 LDS
// tile — both global streams stay coalesced (the naive per-element version
// measured 0.76 TB/s; this is a classic tiled transpose).
__global__ __launch_bounds__(256) void k_permute_krsc_rsck(
    const bf16* __restrict__ src, bf16* __restrict__ dst,
    const int* __restrict__ meta, int nconv) {
  __shared__ bf16 tile[32][33];
  const int ci = blockIdx.y;
  if (ci >= nconv) return;
  const int soff = meta[ci * 4 + 0], doff = meta[ci * 4 + 1];
  const int nelem = meta[ci * 4 + 2];
  const int K = meta[ci * 4 + 3] >> 16, C = meta[ci * 4 + 3] & 0xffff;
  const int RS = nelem / (K * C);
  const int ktiles = (K + 31) / 32, ctiles = (C + 31) / 32;
  const int tiles_per_rs = ktiles * ctiles;
  const int total_tiles = RS * tiles_per_rs;
  // 256 threads = 8 rows of 32 (each thread loads 4 rows)
  const int tc = threadIdx.x & 31, tr = threadIdx.x >> 5;
  for (int t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    int rs = t / tiles_per_rs, rem = t % tiles_per_rs;
    int k0 = (rem / ctiles) * 32, c0 = (rem % ctiles) * 32;
    const bf16* s = src + soff + (long)rs * C;  // row ko: + ko*RS*C
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int ko = k0 + tr + i * 8, c = c0 + tc;
      tile[tr + i * 8][tc] = (ko < K && c < C)
          ? s[(long)ko * RS * C + c] : (bf16)0.f;
    }
    __syncthreads();
    bf16* d = dst + doff + (long)rs * C * K;  // row c: + c*K
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int c = c0 + tr + i * 8, ko = k0 + tc;
      if (c < C && ko < K) d[(long)c * K + ko] = tile[tc][tr + i * 8];
    }
    __syncthreads();
  }
}

// --------------------------------------------------- gradient divergence ---
// sumsq += Σ (g−prev)²; prev ← g   (flat f32), then finalize adds sqrt.
// float4-vectorized main body (the probe moves 3×45 MB per ResNet18 step —
// the scalar version ran at ~2.1 TB/s; engine-flat trace r02); scalar tail.
__global__ __launch_bounds__(256) void k_gdiv_partial(
    const float* __restrict__ g, float* __restrict__ prev,
    float* __restrict__ sumsq, long n) {
  float a = 0.f;
  const long n4 = n >> 2;
  const float4* g4 = (const float4*)g;
  float4* p4 = (float4*)prev;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 gv = g4[i], pv = p4[i];
    float d0 = gv.x - pv.x, d1 = gv.y - pv.y;
    float d2 = gv.z - pv.z, d3 = gv.w - pv.w;
    p4[i] = gv;
    a += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += (long)gridDim.x * blockDim.x) {
    float d = g[i] - prev[i];
    prev[i] = g[i];
    a += d * d;
  }
  a = wave_reduce_sum(a);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(sumsq, ws[0] + ws[1] + ws[2] + ws[3]);
}

// -------------------------------------------- fused u8 batch normalize ----
// uint8 NCHW batch -> normalized bf16 NHWC (channels_last) in ONE pass:
// y = (x/255 - mean)/std  ==  x*scale + shift.  Replaces the eager chain
// to(f32).div_.sub_.div_ + channels_last permute + bf16 cast (~6 torch
// dispatches per step in the training engines' H2D path).
__global__ __launch_bounds__(256) void k_normalize_u8(
    const unsigned char* __restrict__ x, bf16* __restrict__ y, long total,
    int C, long HW, float mean, float std) {
  for (long o = (long)blockIdx.x * blockDim.x + threadIdx.x; o < total;
       o += (long)gridDim.x * blockDim.x) {
    const int c = (int)(o % C);
    const long p = o / C;          // pixel index: n*HW + hw
    const long nidx = p / HW, hw = p % HW;
    // same op order as the reference transform (div, sub, div) so results
    // match the torch chain to the final bf16 rounding
    const float v = ((float)x[(nidx * C + c) * HW + hw] / 255.0f - mean)
                    / std;
    y[o] = (bf16)v;
  }
}

// ------------------------- fused u8 random crop + flip + batch normalize ----
// k_normalize_u8 with RandomCrop(padding=pad) + RandomHorizontalFlip folded
// into the gather address: output pixel (n, ho, wo) reads
//   x[n, c, ho + dy - pad, (flip ? W-1-wo : wo) + dx - pad]
// or the raw byte 0 where that leaves the image (padding happens BEFORE
// the normalize, like torchvision's crop on the uint8 image), then applies
// k_normalize_u8's exact expression, so the two kernels agree bitwise.
// One thread per output pixel looping over c: each plane read is contiguous
// along wo across the wave (flipped or not) and a lane writes its C adjacent
// bf16.  Pixel indices are 32-bit (the binding checks N*C*H*W < 2^31).
//
// Per-sample (dy, dx, flip), RNG = true: a counter-based hash of
// (key, step, n) with key = state[0], step = state[1] — u32 multiply / xor /
// shift / add only; data/augment.py's augment_params is the exact mirror.
// The op leaves state[1] = step + 1 behind so a replayed hipGraph walks the
// stream with no host help.  Two launches: this kernel only READS state, and
// the one-thread k_augment_step_inc behind it on the stream bumps the
// counter — every thread sees the same step by construction.  The
// single-launch last-block-done form (one returning atomic ticket per block
// on one word, last ticket writes step + 1) was built and measured first:
// the device-scope tickets serialise at ~37 ns each — +3.6 us at 256 blocks,
// +145 us at 4096 — against ~1.8 us for the extra dispatch.
// RNG = false: params[n] = dy | dx << 8 | flip << 16 (replay of a recorded
// augmentation); state is not touched.  Offsets outside [0, 2*pad] are
// memory-safe: the window test sends them to the padding value.
DEV unsigned aug_fmix32(unsigned h) {  // murmur3 finaliser
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

template <bool RNG>
__global__ __launch_bounds__(256) void k_augment_normalize_u8(
    const unsigned char* __restrict__ x, bf16* __restrict__ y,
    const unsigned long long* __restrict__ state,
    const int* __restrict__ params, unsigned npix, int C, int H, int W,
    int pad, int do_flip, float mean, float std) {
  unsigned seed = 0;
  if (RNG) {
    const unsigned long long key = state[0], step = state[1];
    seed = aug_fmix32(aug_fmix32(aug_fmix32((unsigned)key) ^
                                 (unsigned)(key >> 32)) ^ (unsigned)step);
  }
  const unsigned HW = (unsigned)H * (unsigned)W;
  const unsigned range = 2u * (unsigned)pad + 1u;
  const float vpad = (0.0f / 255.0f - mean) / std;  // a raw 0 byte
  for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix;
       p += gridDim.x * blockDim.x) {
    const unsigned n = p / HW, hw = p - n * HW;
    const int ho = (int)(hw / (unsigned)W), wo = (int)(hw - ho * W);
    int dy, dx, fl;
    if (RNG) {
      const unsigned t = aug_fmix32(seed ^ (n * 0x9e3779b1u));
      dy = (int)__umulhi(aug_fmix32(t + 0x85ebca77u), range);
      dx = (int)__umulhi(aug_fmix32(t + 2u * 0x85ebca77u), range);
      fl = do_flip ? (int)(aug_fmix32(t + 3u * 0x85ebca77u) >> 31) : 0;
    } else {
      const int q = params[n];
      dy = q & 0xff;
      dx = (q >> 8) & 0xff;
      fl = (q >> 16) & 1;
    }
    const int hi = ho + dy - pad;
    const int wi = (fl ? W - 1 - wo : wo) + dx - pad;
    const bool in = (unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W;
    const unsigned char* src =
        x + (size_t)n * C * HW + (in ? (unsigned)(hi * W + wi) : 0u);
    bf16* dst = y + (size_t)p * C;
    // 4 plane loads in flight per lane (one dependent load per trip left
    // the C = 3 case three load latencies deep).  Padding pixels and
    // channels past C re-read a valid byte and drop it, so no load sits
    // behind a branch.
    for (int c0 = 0; c0 < C; c0 += 4) {
      unsigned char b[4];
#pragma unroll
      for (int e = 0; e < 4; e++)
        b[e] = src[(size_t)min(c0 + e, C - 1) * HW];
#pragma unroll
      for (int e = 0; e < 4; e++) {
        // k_normalize_u8's expression (div, sub, div).  The padding select
        // sits on the RESULT: selecting the byte let the compiler sink the
        // select between the multiply and the subtract, which blocked the
        // fma contraction k_normalize_u8 gets and broke bitwise agreement.
        const float v = ((float)b[e] / 255.0f - mean) / std;
        if (c0 + e < C) dst[c0 + e] = (bf16)(in ? v : vpad);
      }
    }
  }
}

__global__ void k_augment_step_inc(unsigned long long* state) {
  state[1] += 1;
}

__global__ void k_gdiv_finalize(float* __restrict__ sumsq,
                                float* __restrict__ out, int skip_first) {
  if (!skip_first) out[0] += sqrtf(sumsq[0]);
  sumsq[0] = 0.f;
}

// ------------------------------------------------------------- launchers --
static inline int gsz(long total, int block = 256, int cap = 0) {
  static const int dflt_cap = (int)env_long("HZ_GSZ_CAP", 4096);
  if (cap == 0) cap = dflt_cap;
  long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

static int g_det_kernels = 0;

// Grid of the row-split kernels: blockIdx.x walks `xext` channel blocks or
// slabs, blockIdx.y walks msplit chunks of mchunk rows.  msplit fills a
// `budget` of blocks, capped at `cap` (0 = no cap) and at one split per
// `rows_min` rows (0 = no floor); deterministic mode (where `det_single`)
// keeps one split, i.e. a fixed cross-block reduction order.
struct MSplitGrid {
  dim3 grid;
  long mchunk;
};

static MSplitGrid msplit_grid(long M, int xext, int budget, long cap,
                              long rows_min, bool det_single) {
  long msplit = max(1, budget / xext);
  if (cap > 0) msplit = min(msplit, cap);
  if (rows_min > 0)
    msplit = min(msplit, max((long)1, (M + rows_min - 1) / rows_min));
  if (det_single && g_det_kernels) msplit = 1;
  long mchunk = (M + msplit - 1) / msplit;
  msplit = (M + mchunk - 1) / mchunk;
  return {dim3(xext, (unsigned)msplit), mchunk};
}

// the scalar reduce-style kernels: 64-channel columns, <= 768 blocks,
// <= 256 splits
static MSplitGrid scalar_reduce_grid(long M, int C, bool det_single = true) {
  return msplit_grid(M, (C + 63) / 64, 768, 256, 0, det_single);
}

// Runtime value -> compile-time constant: f receives
// std::integral_constant<int, MASK> for mask_mode 0..4 (anything else is 0).
template <class F>
static void with_mask(int mask_mode, F&& f) {
  switch (mask_mode) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

// act 0..2 (anything else is 0) as std::integral_constant<int, ACT>
template <class F>
static void with_act(int act, F&& f) {
  if (act == 1) f(std::integral_constant<int, 1>{});
  else if (act == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 0>{});
}

// (act, training) as (integral_constant<int, ACT>, bool_constant<TRAIN>)
template <class F>
static void with_act_train(int act, int training, F&& f) {
  auto go = [&](auto tr) { with_act(act, [&](auto ac) { f(ac, tr); }); };
  if (training) go(std::true_type{});
  else go(std::false_type{});
}

// ---- v8 BatchNorm dispatch knobs --------------------------------------------
static int bn_v8_enabled() {
  static const int v = (int)env_long("HZ_BN_V8", 1);
  return v;
}

// v8 wins from M >= ~65k rows (isolated sweep: 3.0 TB/s vs 0.7 at
// M=401k/C=64); below that the scalar kernel's per-channel-column layout is
// faster — per-block setup + atomic volume dominate the short v8 m-loops.
static long bn_v8_m_min() {
  static const long v = env_long("HZ_BN_V8_MMIN", 65536L);
  return v;
}

// m-iterations per thread target for the v8 kernels (controls msplit =
// blocks): more iterations -> fewer blocks -> less per-block epilogue +
// atomic volume, at the cost of m-parallelism.
static int bn_v8_iters() {
  // swept: big-M flat, mid-M 1.5-2.5x faster
  static const int v = (int)env_long("HZ_BN_V8_ITERS", 8);
  return v;
}

// mid-M floor for the C <= 512 full-slab rule (swept: scalar kernel wins
// below ~6k rows there).
static long bn_v8_mid_m() {
  static const long v = env_long("HZ_BN_V8_MIDM", 6000L);
  return v;
}

// channel-slab admission: C > 512 shapes run v8 with blockIdx.x slicing C
// into <=512-channel slabs (keeps >=4 m-rows per block).  Floor swept on
// the r50@224 leftovers (M=1568..6272, C=1024/2048).
static int bn_v8_slab_enabled() {
  static const int v = (int)env_long("HZ_BN_V8_SLAB", 1);
  return v;
}

static long bn_v8_slab_m_min() {
  static const long v = env_long("HZ_BN_V8_SLAB_MMIN", 1024L);
  return v;
}

// largest slab width <= 512 that divides C and keeps 8-channel lanes;
// C itself if no such divisor (then only the full-C rules admit v8).
static int bn_v8_cslab(int C) {
  if (C <= 512) return C;
  for (int ns = (C + 511) / 512; ns <= 64; ns++)
    if (C % ns == 0 && ((C / ns) & 7) == 0) return C / ns;
  return C;
}

// dispatch rule (isolated sweeps, HZ_BN_V8_ITERS grid): v8 wins at
// M >= 65k for any C, at mid M (>= ~6k) for C <= 512, and — via the
// channel-slab grid — down to M >= ~1k for C > 512 (full-C blocks there
// had mstep=1, the slab form keeps the scalar kernel's m-parallelism with
// dwordx4 loads).
static bool bn_v8_pick(long M, int C) {
  if ((C & 7) != 0 || C > 2048 || !bn_v8_enabled()) return false;
  if (M >= bn_v8_m_min()) return true;
  if (C <= 512) return M >= bn_v8_mid_m();
  return bn_v8_slab_enabled() && M >= bn_v8_slab_m_min() &&
         bn_v8_cslab(C) < C;
}

// The c-blocked apply kernels take any C % 8 == 0 whose slab is <= 2048:
// that keeps lpr <= 256 (a C = 8 x large-prime extent has no viable slab
// divisor and would make mstep = 0) — such channel counts fall back to the
// flat elementwise kernel.
static bool bn_apply_v8_ok(int C) {
  return (C & 7) == 0 && bn_v8_cslab(C) <= 2048;
}

// v8 grids: one <=512-channel slab per block (blockIdx.x), m split across
// blockIdx.y so that every thread has >= `iters` rows and the grid reaches
// ~768 blocks on big-M shapes (matching the scalar kernels' fill).
static MSplitGrid bn_v8_grid(long M, int C, int iters, bool det_single,
                             int* cslab_out) {
  int cslab = bn_v8_cslab(C), nslab = C / cslab;
  int lpr = cslab >> 3, mstep = 256 / lpr;
  *cslab_out = cslab;
  return msplit_grid(M, nslab, 768, 0, (long)mstep * iters, det_single);
}

// the reduce kernels' per-block LDS epilogue + atomics reward long m-loops
static MSplitGrid bn_v8_reduce_grid(long M, int C, int* cslab_out) {
  return bn_v8_grid(M, C, bn_v8_iters(), true, cslab_out);
}

// apply has no epilogue and its f32 split-K slab-sum is LATENCY-bound —
// one m-row per thread, i.e. maximum thread parallelism, measured 4x
// faster at the small CIFAR shapes (30.2 -> ~7 us); the 768-block cap
// keeps big-M shapes at the same fill as before.
static MSplitGrid bn_apply_grid(long M, int C, int* cslab_out) {
  return bn_v8_grid(M, C, 1, false, cslab_out);
}

template <bool F32SRC>
static void bn_apply_any(const void* x, const void* res, void* y,
                         void* convout, const float* stats,
                         const float* gamma, const float* beta, float* rmean,
                         float* rvar, float* smean, float* sinvstd, long M,
                         int C, float momentum, float eps, int training,
                         int act, int nsplit, hipStream_t st) {
  if (bn_apply_v8_ok(C)) {
    int cslab;
    MSplitGrid g = bn_apply_grid(M, C, &cslab);
    with_act_train(act, training, [&](auto ac, auto tr) {
      k_bn_apply_v8<F32SRC, ac.value, tr.value><<<g.grid, 256, 0, st>>>(
          x, (const bf16*)res, (bf16*)y, (bf16*)convout, stats, gamma, beta,
          rmean, rvar, smean, sinvstd, M, C, momentum, eps, nsplit, g.mchunk,
          cslab);
    });
    return;
  }
  with_act_train(act, training, [&](auto ac, auto tr) {
    k_bn_apply<F32SRC, ac.value, tr.value>
        <<<gsz(M * (long)C / 8 + 1), 256, 0, st>>>(
            x, (const bf16*)res, (bf16*)y, (bf16*)convout, stats, gamma,
            beta, rmean, rvar, smean, sinvstd, M, C, momentum, eps, nsplit);
  });
}

extern "C" {

void set_kernels_deterministic(int on) { g_det_kernels = on; }

void launch_stats_bf16_det(const void* x, float* stats, long M, int C,
                           hipStream_t st) {
  k_stats_bf16_det<<<(C + 63) / 64, 256, 0, st>>>((const bf16*)x, stats, M,
                                                  C);
}

void launch_bn_apply(const void* x, const void* res, void* y,
                     const float* stats, const float* gamma,
                     const float* beta, float* rmean, float* rvar,
                     float* smean, float* sinvstd, long M, int C,
                     float momentum, float eps, int training, int act,
                     hipStream_t st) {
  bn_apply_any<false>(x, res, y, nullptr, stats, gamma, beta, rmean, rvar,
                      smean, sinvstd, M, C, momentum, eps, training, act, 1,
                      st);
}

void launch_bn_apply_f32(const float* ws, const void* res, void* y,
                         void* convout, const float* stats,
                         const float* gamma, const float* beta, float* rmean,
                         float* rvar, float* smean, float* sinvstd, long M,
                         int C, float momentum, float eps, int training,
                         int act, int nsplit, hipStream_t st) {
  bn_apply_any<true>(ws, res, y, convout, stats, gamma, beta, rmean, rvar,
                     smean, sinvstd, M, C, momentum, eps, training, act,
                     nsplit, st);
}

void launch_stats_reduce(const float* ws, float* stats, long M, int C,
                         int nsplit, hipStream_t st) {
  MSplitGrid g = scalar_reduce_grid(M, C);
  k_stats_reduce<<<g.grid, 256, 0, st>>>(ws, stats, M, C, g.mchunk, nsplit);
}

void launch_cast_f32_bf16(const float* src, void* dst, long n, int nsplit,
                          int accum, hipStream_t st) {
  k_cast_f32_bf16<<<gsz(n / 8 + 1), 256, 0, st>>>(src, (bf16*)dst, n,
                                                   nsplit, accum);
}

void launch_cast_bnact(const float* src, void* dst, long M, int C,
                       int nsplit, int accum, const void* x_up,
                       const void* y_up, const float* smean,
                       const float* sinvstd, const float* gamma,
                       const float* beta, float* sum_dz, float* sum_dzx,
                       int mask_mode, hipStream_t st) {
  if (bn_v8_pick(M, C)) {
    int cslab;
    MSplitGrid g = bn_v8_reduce_grid(M, C, &cslab);
    with_mask(mask_mode, [&](auto mk) {
      k_cast_bnact_v8<mk.value><<<g.grid, 256, 0, st>>>(
          src, (bf16*)dst, M, C, nsplit, accum, (const bf16*)x_up,
          (const bf16*)y_up, smean, sinvstd, gamma, beta, sum_dz, sum_dzx,
          g.mchunk, cslab);
    });
    return;
  }
  MSplitGrid g = scalar_reduce_grid(M, C);
  k_cast_bnact<<<g.grid, 256, 0, st>>>(src, (bf16*)dst, M, C, nsplit, accum,
                                       (const bf16*)x_up, (const bf16*)y_up,
                                       smean, sinvstd, gamma, beta, sum_dz,
                                       sum_dzx, mask_mode, g.mchunk);
}

void launch_bnact_bwd_reduce(const void* dy, const void* yout, const void* x,
                             const float* smean, const float* sinvstd,
                             const float* gamma, const float* beta,
                             float* sum_dz, float* sum_dzx, long M, int C,
                             int mask_mode, hipStream_t st) {
  // sum_dz/sum_dzx must be pre-zeroed (they are accumulated atomically)
  if (bn_v8_pick(M, C)) {
    int cslab;
    MSplitGrid g = bn_v8_reduce_grid(M, C, &cslab);
    with_mask(mask_mode, [&](auto mk) {
      k_bnact_bwd_reduce_v8<mk.value><<<g.grid, 256, 0, st>>>(
          (const bf16*)dy, (const bf16*)yout, (const bf16*)x, smean, sinvstd,
          gamma, beta, sum_dz, sum_dzx, M, C, g.mchunk, cslab);
    });
    return;
  }
  MSplitGrid g = scalar_reduce_grid(M, C);
  k_bnact_bwd_reduce<<<g.grid, 256, 0, st>>>(
      (const bf16*)dy, (const bf16*)yout, (const bf16*)x, smean, sinvstd,
      gamma, beta, sum_dz, sum_dzx, M, C, mask_mode, g.mchunk);
}

void launch_bn_bwd_apply(const void* dy, const void* yout, const void* x,
                         const float* smean, const float* sinvstd,
                         const float* gamma, const float* beta,
                         const float* sum_dz, const float* sum_dzx,
                         void* dconv, void* dres, long M, int C,
                         int mask_mode, hipStream_t st) {
  if (bn_apply_v8_ok(C)) {
    int cslab;
    MSplitGrid g = bn_apply_grid(M, C, &cslab);
    with_mask(mask_mode, [&](auto mk) {
      k_bn_bwd_apply_v8<mk.value><<<g.grid, 256, 0, st>>>(
          (const bf16*)dy, (const bf16*)yout, (const bf16*)x, smean, sinvstd,
          gamma, beta, sum_dz, sum_dzx, (bf16*)dconv, (bf16*)dres, M, C,
          g.mchunk, cslab);
    });
    return;
  }
  with_mask(mask_mode, [&](auto mk) {
    k_bn_bwd_apply<mk.value><<<gsz(M * (long)C / 8 + 1), 256, 0, st>>>(
        (const bf16*)dy, (const bf16*)yout, (const bf16*)x, smean, sinvstd,
        gamma, beta, sum_dz, sum_dzx, (bf16*)dconv, (bf16*)dres, M, C);
  });
}

// ---- channel-owner BN dispatch ---------------------------------------------
// Runtime switch (set_bn_owner) + env knobs.  The owner kernels run on
// C/(4*lpr) workgroups, so they only pay while one workgroup covers all M
// rows quickly: M limits per direction (HZ_BN_OWNER_FWD_MMAX /
// HZ_BN_OWNER_BWD_MMAX) and lanes-per-row (HZ_BN_OWNER_FWD_LPR /
// HZ_BN_OWNER_BWD_LPR; wider = full cache lines per row, narrower = more
// workgroups) come from scripts/gpu_bn_owner_sweep.py — docs/TUNING.md.
static int g_bn_owner = (int)env_long("HZ_BN_OWNER", 1);  // read at load
static long g_owner_fwd_launches = 0, g_owner_bwd_launches = 0;

void set_kernels_bn_owner(int on) { g_bn_owner = on; }
int kernels_bn_owner() { return g_bn_owner; }
void bn_owner_launch_counts(long* fwd, long* bwd) {
  *fwd = g_owner_fwd_launches;
  *bwd = g_owner_bwd_launches;
}

// LDS image budget of the forward kernel (static LDS + this stays inside
// the 64 KB a kernel gets without opting in to more).
constexpr long kOwnerFwdLdsBytes = 60 * 1024;

// widest lanes-per-row <= want (power of two, <= 8) whose channel slice
// divides C; C % 8 == 0 guarantees lpr = 2 fits.
static int owner_lpr(int C, int want) {
  int lpr = 8;
  while (lpr > 1 && (lpr > want || C % (4 * lpr) != 0)) lpr >>= 1;
  return lpr;
}

// Returns the lanes-per-row to launch with, or 0 when the shape keeps the
// two-kernel path.  lpr_req > 0 pins the width (sweeps); it is still
// narrowed to fit C and the LDS image.
int bn_owner_fwd_pick(long M, int C, int lpr_req) {
  // swept: wins at M <= 512 (layer3/4 of the flagship), ties the pair at
  // M = 1024 where 16 workgroups stream 4 MB of slabs; 2 lanes per row
  // won at every winning shape
  static const long mmax = env_long("HZ_BN_OWNER_FWD_MMAX", 512);
  static const int want = (int)env_long("HZ_BN_OWNER_FWD_LPR", 2);
  if (!g_bn_owner || g_det_kernels || (C & 7) != 0 || M < 1) return 0;
  if (lpr_req <= 0 && M > mmax) return 0;
  int lpr = owner_lpr(C, lpr_req > 0 ? lpr_req : want);
  while (lpr > 1 && M * lpr * 16 > kOwnerFwdLdsBytes) lpr >>= 1;
  if (M * lpr * 16 > kOwnerFwdLdsBytes) return 0;
  return lpr;
}

int bn_owner_bwd_pick(long M, int C, int lpr_req) {
  // swept: wins up to M = 1024, loses 2x at M = 4096 (C = 64 leaves 8-16
  // workgroups reading 8 bytes of every 128-byte row).  Lanes per row
  // (0 = auto): narrow rows at large M for more workgroups, full lines at
  // small M where C/32 workgroups are still plenty.
  static const long mmax = env_long("HZ_BN_OWNER_BWD_MMAX", 1024);
  static const int want = (int)env_long("HZ_BN_OWNER_BWD_LPR", 0);
  if (!g_bn_owner || g_det_kernels || (C & 7) != 0 || M < 1) return 0;
  if (M > (lpr_req > 0 ? (long)1 << 24 : mmax)) return 0;
  // swept: M*C = 256 Ki still wins (M=1024/C=256 8.3 vs 9.1 us, M=512/
  // C=512 6.4 vs 7.0), M=1024/C=512 loses 2x (15.4 vs 7.7 us: the pair
  // fills the chip there) and cost layer4 at batch 1024 0.6% of its step
  static const long emax = env_long("HZ_BN_OWNER_BWD_EMAX", 262144);
  if (lpr_req <= 0 && M * C > emax) return 0;
  int w = lpr_req > 0 ? lpr_req : want;
  if (w <= 0) w = (int)max((long)2, min((long)8, 1024 / M));
  return owner_lpr(C, w);
}

void launch_bn_fwd_owner(const float* ws, const void* res, void* y,
                         void* convout, const float* gamma,
                         const float* beta, float* rmean, float* rvar,
                         float* smean, float* sinvstd, long M, int C,
                         float momentum, float eps, int act, int nsplit,
                         int lpr, hipStream_t st) {
  const int rl = 256 / lpr;
  int zg = 1;
  if (M < rl) zg = (int)max((long)1, min((long)nsplit, rl / M));
  const size_t lds = (size_t)M * zg * lpr * 16;
  dim3 grid(C / (4 * lpr));
  with_act(act, [&](auto ac) {
    k_bn_fwd_owner<ac.value><<<grid, 256, lds, st>>>(
        ws, (const bf16*)res, (bf16*)y, (bf16*)convout, gamma, beta, rmean,
        rvar, smean, sinvstd, (int)M, C, momentum, eps, nsplit, lpr, zg);
  });
  g_owner_fwd_launches++;
}

void launch_bn_bwd_owner(const void* dy, const void* yout, const void* x,
                         const float* smean, const float* sinvstd,
                         const float* gamma, const float* beta,
                         float* sum_dz, float* sum_dzx, void* dconv,
                         void* dres, long M, int C, int mask_mode, int lpr,
                         hipStream_t st) {
  dim3 grid(C / (4 * lpr));
  with_mask(mask_mode, [&](auto mk) {
    k_bn_bwd_owner<mk.value><<<grid, 256, 0, st>>>(
        (const bf16*)dy, (const bf16*)yout, (const bf16*)x, smean, sinvstd,
        gamma, beta, sum_dz, sum_dzx, (bf16*)dconv, (bf16*)dres, (int)M, C,
        lpr);
  });
  g_owner_bwd_launches++;
}

void launch_dw_fwd(const void* x, const void* w, void* y, float* stats,
                   int Nb, int H, int W, int C, int Ho, int Wo, int R,
                   int S, int str, int pad, hipStream_t st) {
  MSplitGrid g = scalar_reduce_grid((long)Nb * Ho * Wo, C);
  k_dw_fwd<<<g.grid, 256, 0, st>>>((const bf16*)x, (const bf16*)w, (bf16*)y,
                                   stats, Nb, H, W, C, Ho, Wo, R, S, str,
                                   pad, g.mchunk);
}

void launch_dw_dgrad(const void* dz, const void* w, void* dx, int Nb, int H,
                     int W, int C, int Ho, int Wo, int R, int S, int str,
                     int pad, hipStream_t st) {
  // no cross-block reduction here: deterministic mode keeps the full split
  MSplitGrid g = scalar_reduce_grid((long)Nb * H * W, C, false);
  k_dw_dgrad<<<g.grid, 256, 0, st>>>((const bf16*)dz, (const bf16*)w,
                                     (bf16*)dx, Nb, H, W, C, Ho, Wo, R, S,
                                     str, pad, g.mchunk);
}

void launch_dw_wgrad(const void* x, const void* dz, float* dw, int Nb,
                     int H, int W, int C, int Ho, int Wo, int R, int S,
                     int str, int pad, hipStream_t st) {
  MSplitGrid g = msplit_grid((long)Nb * Ho * Wo, (C + 63) / 64, 512, 64, 0,
                             true);
  k_dw_wgrad<<<g.grid, 256, 0, st>>>((const bf16*)x, (const bf16*)dz, dw, Nb,
                                     H, W, C, Ho, Wo, R, S, str, pad,
                                     g.mchunk);
}

void launch_maxpool_fwd(const void* x, void* y, unsigned char* idx, int Nb,
                        int H, int W, int C, int Hp, int Wp, hipStream_t st) {
  if ((C & 7) == 0)
    k_maxpool_fwd_v8<<<gsz((long)Nb * Hp * Wp * (C >> 3)), 256, 0, st>>>(
        (const bf16*)x, (bf16*)y, idx, Nb, H, W, C, Hp, Wp);
  else
    k_maxpool_fwd<<<gsz((long)Nb * Hp * Wp * C), 256, 0, st>>>(
        (const bf16*)x, (bf16*)y, idx, Nb, H, W, C, Hp, Wp);
}

void launch_maxpool_bwd(const void* dy, const unsigned char* idx, void* dx,
                        int Nb, int H, int W, int C, int Hp, int Wp,
                        hipStream_t st) {
  if ((C & 7) == 0)
    k_maxpool_bwd_v8<<<gsz((long)Nb * H * W * (C >> 3)), 256, 0, st>>>(
        (const bf16*)dy, idx, (bf16*)dx, Nb, H, W, C, Hp, Wp);
  else
    k_maxpool_bwd<<<gsz((long)Nb * H * W * C), 256, 0, st>>>(
        (const bf16*)dy, idx, (bf16*)dx, Nb, H, W, C, Hp, Wp);
}

void launch_avgpool_fwd(const void* x, void* y, int Nb, int HW, int C,
                        hipStream_t st) {
  k_avgpool_fwd<<<gsz((long)Nb * C), 256, 0, st>>>((const bf16*)x, (bf16*)y,
                                                   Nb, HW, C);
}

void launch_avgpool_bwd(const void* dy, void* dx, int Nb, int HW, int C,
                        hipStream_t st) {
  k_avgpool_bwd<<<gsz((long)Nb * HW * C), 256, 0, st>>>((const bf16*)dy,
                                                        (bf16*)dx, Nb, HW, C);
}

void launch_linear_fwd(const void* x, const void* w, const float* b, float* y,
                       int B, int In, int Out, hipStream_t st) {
  k_linear_fwd<<<(B + 3) / 4, 256, 0, st>>>((const bf16*)x, (const bf16*)w,
                                            b, y, B, In, Out);
}

void launch_linear_bwd(const float* dy, const void* x, const void* w,
                       void* dx, float* dw, float* db, int B, int In, int Out,
                       int accum, hipStream_t st) {
  if (dx)
    k_linear_bwd_dx<<<gsz((long)B * In), 256, 0, st>>>(dy, (const bf16*)w,
                                                       (bf16*)dx, B, In, Out);
  if (Out <= 16 && B <= 128)
    k_linear_bwd_dw_small<<<gsz((long)In), 256, 0, st>>>(
        dy, (const bf16*)x, dw, db, B, In, Out, accum);
  else if (Out <= 16 && !g_det_kernels) {
    int bsplit = (B + 127) / 128;
    if (!accum) {  // fresh output buffers: atomics need zeroed targets
      hipError_t e1 = hipMemsetAsync(dw, 0, sizeof(float) * (long)Out * In,
                                     st);
      hipError_t e2 = (db != nullptr)
          ? hipMemsetAsync(db, 0, sizeof(float) * Out, st) : hipSuccess;
      if (e1 != hipSuccess || e2 != hipSuccess)
        fprintf(stderr, "[horizonml] linear-wgrad memset failed: %s\n",
                hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    }
    dim3 grid((In + 255) / 256, bsplit);
    k_linear_bwd_dw_bsplit<<<grid, 256, 0, st>>>(dy, (const bf16*)x, dw,
                                                 db, B, In, Out, 128);
  } else
    k_linear_bwd_dw<<<gsz((long)Out * In), 256, 0, st>>>(
        dy, (const bf16*)x, dw, db, B, In, Out, accum);
}

void launch_ce_fwd_bwd(const float* logits, const long* target, float* loss,
                       float* dlogits, int B, int NC, hipStream_t st) {
  if (g_det_kernels)
    k_ce_fwd_bwd_det<<<1, 256, 0, st>>>(logits, target, loss, dlogits, B,
                                        NC);
  else
    k_ce_fwd_bwd<<<gsz(B), 256, 0, st>>>(logits, target, loss, dlogits, B,
                                         NC);
}

void launch_ce_ls_fwd_bwd(const float* logits, const long* target,
                          float* loss, float* dlogits, int B, int NC,
                          float eps, hipStream_t st) {
  if (g_det_kernels)
    k_ce_ls_fwd_bwd_det<<<1, 256, 0, st>>>(logits, target, loss, dlogits, B,
                                           NC, eps);
  else
    k_ce_ls_fwd_bwd<<<gsz(B), 256, 0, st>>>(logits, target, loss, dlogits, B,
                                            NC, eps);
}

void launch_adam_step(float* master, float* grad, float* m, float* v,
                      void* shadow, float* step_t, long n, float lr,
                      float b1, float b2, float eps, float wd, int zero_grad,
                      float* extra_zero, long n_extra, const void* gsrc,
                      float gscale, float* prev, float* sumsq, float* divout,
                      hipStream_t st) {
  k_inc_step<<<1, 1, 0, st>>>(step_t);
  k_adam_step<<<gsz(n), 256, 0, st>>>(master, grad, m, v, (bf16*)shadow,
                                      step_t, n, lr, b1, b2, eps, wd,
                                      zero_grad, extra_zero, n_extra,
                                      (const bf16*)gsrc, gscale, prev,
                                      sumsq);
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

void launch_sgd_step(float* master, float* grad, float* mom, void* shadow,
                     long n, float lr, float mu, float wd, int zero_grad,
                     const void* gsrc, float gscale, float* prev,
                     float* sumsq, float* divout, hipStream_t st) {
  k_sgd_step<<<gsz(n), 256, 0, st>>>(master, grad, mom, (bf16*)shadow, n, lr,
                                     mu, wd, zero_grad, (const bf16*)gsrc,
                                     gscale, prev, sumsq);
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

// Scheduled / extended forms.  Adam bumps its own step_t exactly as above
// (no added dispatch); SGD bumps `step_t` with the same one-thread kernel
// only when it has a table to index (two-launch scheme, see
// k_augment_normalize_u8's counter).
void launch_adam_step_ex(float* master, float* grad, float* m, float* v,
                         void* shadow, float* step_t, long n, float lr,
                         float b1, float b2, float eps, float wd,
                         int zero_grad, float* extra_zero, long n_extra,
                         const void* gsrc, float gscale, float* prev,
                         float* sumsq, float* divout, const float* lr_table,
                         long T, float* lr_out, int decoupled,
                         hipStream_t st) {
  k_inc_step<<<1, 1, 0, st>>>(step_t);
#define LA(D) k_adam_step_ex<D><<<gsz(n), 256, 0, st>>>( \
    master, grad, m, v, (bf16*)shadow, step_t, n, lr, b1, b2, eps, wd, \
    zero_grad, extra_zero, n_extra, (const bf16*)gsrc, gscale, prev, sumsq, \
    lr_table, T, lr_out)
  if (decoupled) LA(true); else LA(false);
#undef LA
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

void launch_sgd_step_ex(float* master, float* grad, float* mom, void* shadow,
                        long n, float lr, float mu, float wd, int zero_grad,
                        const void* gsrc, float gscale, float* prev,
                        float* sumsq, float* divout, float* step_t,
                        const float* lr_table, long T, float* lr_out,
                        int nesterov, hipStream_t st) {
  if (lr_table != nullptr) k_inc_step<<<1, 1, 0, st>>>(step_t);
#define LS(N) k_sgd_step_ex<N><<<gsz(n), 256, 0, st>>>( \
    master, grad, mom, (bf16*)shadow, n, lr, mu, wd, zero_grad, \
    (const bf16*)gsrc, gscale, prev, sumsq, step_t, lr_table, T, lr_out)
  if (nesterov) LS(true); else LS(false);
#undef LS
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

// Segmented forms: the counter bumps are those of the *_ex launchers.
void launch_seg_norms(const float* master, const float* grad,
                      const void* gsrc, float gscale, const int* chunks,
                      int nchunks, const int* seg_meta, int nseg,
                      float* partials, float* seg_norms, float* seg_mul,
                      float* norm_out, float wd, float max_norm, int lars,
                      float eta, hipStream_t st) {
  k_seg_sumsq_partial<<<nchunks, 256, 0, st>>>(master, grad,
                                               (const bf16*)gsrc, gscale,
                                               chunks, partials, lars);
  k_seg_finalize<<<1, 64 * kSegFinWaves, 0, st>>>(partials, seg_meta, nseg, wd, max_norm,
                                    lars, eta, seg_norms, seg_mul, norm_out);
}

void launch_adam_step_seg(float* master, float* grad, float* m, float* v,
                          void* shadow, float* step_t, float lr, float b1,
                          float b2, float eps, int zero_grad,
                          float* extra_zero, long n_extra, const void* gsrc,
                          float gscale, float* prev, float* sumsq,
                          float* divout, const float* lr_table, long T,
                          float* lr_out, int decoupled, const int* chunks,
                          int nchunks, const float* seg_mul, hipStream_t st) {
  k_inc_step<<<1, 1, 0, st>>>(step_t);
#define LA(D) k_adam_step_seg<D><<<nchunks, 256, 0, st>>>( \
    master, grad, m, v, (bf16*)shadow, step_t, lr, b1, b2, eps, zero_grad, \
    extra_zero, n_extra, (const bf16*)gsrc, gscale, prev, sumsq, lr_table, \
    T, lr_out, chunks, seg_mul)
  if (decoupled) LA(true); else LA(false);
#undef LA
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

void launch_sgd_step_seg(float* master, float* grad, float* mom, void* shadow,
                         float lr, float mu, int zero_grad, const void* gsrc,
                         float gscale, float* prev, float* sumsq,
                         float* divout, float* step_t, const float* lr_table,
                         long T, float* lr_out, int nesterov,
                         const int* chunks, int nchunks, const float* seg_mul,
                         hipStream_t st) {
  if (lr_table != nullptr) k_inc_step<<<1, 1, 0, st>>>(step_t);
#define LS(N) k_sgd_step_seg<N><<<nchunks, 256, 0, st>>>( \
    master, grad, mom, (bf16*)shadow, lr, mu, zero_grad, (const bf16*)gsrc, \
    gscale, prev, sumsq, step_t, lr_table, T, lr_out, chunks, seg_mul)
  if (nesterov) LS(true); else LS(false);
#undef LS
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

// Live-range forms: the counter bumps are those of the *_ex launchers.
void launch_adam_step_live(float* master, float* grad, float* m, float* v,
                           void* shadow, float* step_t, float lr, float b1,
                           float b2, float eps, int zero_grad,
                           float* extra_zero, long n_extra, const void* gsrc,
                           float gscale, float* prev, float* sumsq,
                           float* divout, const float* lr_table, long T,
                           float* lr_out, const int* live, int nchunks,
                           hipStream_t st) {
  k_inc_step<<<1, 1, 0, st>>>(step_t);
  k_adam_step_live<<<nchunks, 256, 0, st>>>(
      master, grad, m, v, (bf16*)shadow, step_t, lr, b1, b2, eps, zero_grad,
      extra_zero, n_extra, (const bf16*)gsrc, gscale, prev, sumsq, lr_table,
      T, lr_out, (const int4*)live);
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

void launch_sgd_step_live(float* master, float* grad, float* mom,
                          void* shadow, float lr, float mu, int zero_grad,
                          const void* gsrc, float gscale, float* prev,
                          float* sumsq, float* divout, float* step_t,
                          const float* lr_table, long T, float* lr_out,
                          int nesterov, const int* live, int nchunks,
                          hipStream_t st) {
  if (lr_table != nullptr) k_inc_step<<<1, 1, 0, st>>>(step_t);
#define LS(N) k_sgd_step_live<N><<<nchunks, 256, 0, st>>>( \
    master, grad, mom, (bf16*)shadow, lr, mu, zero_grad, (const bf16*)gsrc, \
    gscale, prev, sumsq, step_t, lr_table, T, lr_out, (const int4*)live)
  if (nesterov) LS(true); else LS(false);
#undef LS
  if (prev != nullptr)
    k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, divout, 0);
}

void launch_permute_krsc_rsck(const void* src, void* dst, const int* meta,
                              int nconv, int max_elem, hipStream_t st) {
  dim3 grid(gsz((long)max_elem, 1024), nconv);  // tiles grid-stride per conv
  k_permute_krsc_rsck<<<grid, 256, 0, st>>>((const bf16*)src, (bf16*)dst,
                                            meta, nconv);
}

void launch_grad_divergence(const float* g, float* prev, float* sumsq,
                            float* out, long n, int skip_first,
                            hipStream_t st) {
  k_gdiv_partial<<<gsz(n >> 2), 256, 0, st>>>(g, prev, sumsq, n);
  k_gdiv_finalize<<<1, 1, 0, st>>>(sumsq, out, skip_first);
}

void launch_normalize_u8(const void* x, void* y, long total, int C, long HW,
                         float mean, float std, hipStream_t st) {
  k_normalize_u8<<<gsz(total), 256, 0, st>>>((const unsigned char*)x,
                                             (bf16*)y, total, C, HW, mean,
                                             std);
}

// params == nullptr: RNG mode (state = {key, step}; a second one-thread
// launch advances the step on the device); otherwise explicit per-sample
// parameters, state unused.
void launch_augment_normalize_u8(const void* x, void* y, void* state,
                                 const int* params, long N, int C, int H,
                                 int W, int pad, int flip, float mean,
                                 float std, hipStream_t st) {
  const long npix = N * H * W;
  const int grid = gsz(npix);
  if (params == nullptr) {
    k_augment_normalize_u8<true><<<grid, 256, 0, st>>>(
        (const unsigned char*)x, (bf16*)y, (const unsigned long long*)state,
        nullptr, (unsigned)npix, C, H, W, pad, flip, mean, std);
    k_augment_step_inc<<<1, 1, 0, st>>>((unsigned long long*)state);
  } else
    k_augment_normalize_u8<false><<<grid, 256, 0, st>>>(
        (const unsigned char*)x, (bf16*)y, nullptr, params, (unsigned)npix,
        C, H, W, pad, flip, mean, std);
}

}  // extern "C"
