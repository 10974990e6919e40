// GroupNorm for gfx950 (MI355X, CDNA4).  docs/KERNELS.md, "GroupNorm".
//
//   x̂ = (x − μ[n,g])·rstd[n,g],  y = act(γ·x̂ + β [+ residual])
//   g = dy·mask(y);  s1 = Σ g·γ, s2 = Σ g·γ·x̂ per (n, group)
//   dconv = rstd·(g·γ − (s1 + x̂·s2)/(HW·Cg)),  dres = g
//   dβ = Σ g, dγ = Σ g·x̂ per channel
//
// x, residual, y, dy, dconv, dres are bf16 NHWC [N][HW][C]; the forward also
// takes split-K conv slabs [nsplit][N·HW][C] f32, sums them in slab order and
// stores the bf16 conv output in the same pass.  Statistics are taken from
// the bf16-ROUNDED values, the ones backward reads again.  G groups of
// Cg = C/G adjacent channels, Cg in {2, 4, 8, 16, 32, 64}, C % 8 == 0.
//
// Ownership: a workgroup of 256 threads owns one sample n and one slab of
// 8·lpr adjacent channels (lpr lanes per row, 8..64) over rows [r0, r1) of
// that sample: all HW rows in the one-launch form, one chunk of them
// (blockIdx.z) in the split form.  Thread tid holds channels
// slab + 8·(tid % lpr) .. +7 of rows r0 + tid/lpr + k·(256/lpr): one 16-byte
// access per row.  A slab is a whole number of groups (Cg ≤ 64 = 8·8).
//
// Reduction order, the same for every sample whatever the batch holds: the
// thread's rows ascending; the lane's 8 channels pairwise up to the group
// (Cg ≤ 8) and then across the group's Cg/8 adjacent lanes by xor shuffles
// (Cg ≥ 16); the wave's rows by xor shuffles 32 .. lpr; the four waves
// through LDS in wave order 0..3; in the split form the chunks in chunk
// order.  Nothing here has an atomic, so default and deterministic mode run
// the same code.
//
// Variance is two-pass: the mean, then Σ(x − μ)² over the same rows, which
// are kept in LDS between the passes (and for the apply pass) as far as the
// budget GN_RES_ITERS goes and re-read from global, L2-hot, beyond it.  The
// split form merges per-chunk (mean, M2) pairs by Chan's update.
//
// EXEC rule: every shuffle and barrier runs with EXEC all ones.  Loop trip
// counts and roles are block-uniform; rows ≥ r1 and channels ≥ C are ZEROS
// that enter the sums with a zero weight, never masked lanes or early exits.
#include "common.h"

#include <algorithm>

constexpr int GN_THREADS = 256;
// Rows a thread keeps in LDS, 16 bytes each: 13·4 KB = 52 KB of dynamic LDS
// next to the 8 KB fold buffer, under the 64 KB a kernel gets without opting
// in and two workgroups per CU of gfx950's 160 KB.  Backward keeps g and x:
// half as many rows.
constexpr int GN_RES_ITERS = 13;

struct GnP {
  int HW, C, G, cgs;  // rows per sample, channels, groups, log2(C / G)
  int lpr;            // lanes per row; the slab is 8·lpr channels
  int chunk, Z;       // rows per workgroup, workgroups per (sample, slab)
  int resident;       // row iterations kept in LDS
  int nsplit;         // F32SRC: slabs to sum
  long sstride;       // F32SRC: floats per slab
  float eps;
};

// A thread's place in its workgroup.
struct GnT {
  int tid, lane, wave;
  int cl, rr, rpp;  // lane of the row, first row, rows per pass
  int c0;           // first of the thread's 8 channels
  bool cok;         // C % 8 == 0: the 8 channels are all inside or all outside
};

DEV GnT gn_place(const GnP& p) {
  GnT t;
  t.tid = threadIdx.x;
  t.lane = t.tid & 63;
  t.wave = __builtin_amdgcn_readfirstlane(t.tid >> 6);
  t.cl = t.tid & (p.lpr - 1);
  t.rr = t.tid / p.lpr;
  t.rpp = GN_THREADS / p.lpr;
  t.c0 = blockIdx.x * 8 * p.lpr + t.cl * 8;
  t.cok = t.c0 < p.C;
  return t;
}

// Per-channel values of a lane -> the total of each channel pair's GROUP, in
// every lane of the group (broadcast form: s[j] belongs to channels 2j,
// 2j+1).  Cg is block-uniform.
DEV void gn_group_fold(const float (&v)[8], int Cg, float (&s)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = v[2 * j] + v[2 * j + 1];
  if (Cg >= 4) {
    const float a = s[0] + s[1], b = s[2] + s[3];
    s[0] = s[1] = a;
    s[2] = s[3] = b;
  }
  if (Cg >= 8) {
    float a = s[0] + s[2];
    for (int off = 1; off < (Cg >> 3); off <<= 1)
      a += __shfl_xor(a, off, 64);
    s[0] = s[1] = s[2] = s[3] = a;
  }
}

// Σ over the workgroup's rows of NV per-lane values, left in every thread
// that holds the same channels.  red: 4·8·64 floats.
template <int NV>
DEV void gn_block_sum(float (&v)[NV], const GnT& t, int lpr, float* red) {
  for (int off = 32; off >= lpr; off >>= 1) {
#pragma unroll
    for (int e = 0; e < NV; e++) v[e] += __shfl_xor(v[e], off, 64);
  }
  __syncthreads();  // the previous fold's reads of red are done
  if (t.lane < lpr) {
#pragma unroll
    for (int e = 0; e < NV; e++) red[(t.wave * NV + e) * 64 + t.lane] = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NV; e++) {
    float s = red[e * 64 + t.cl];
    s += red[(NV + e) * 64 + t.cl];
    s += red[(2 * NV + e) * 64 + t.cl];
    s += red[(3 * NV + e) * 64 + t.cl];
    v[e] = s;
  }
}

// One value per group of the lane -> dst[G] of the sample; `w` picks the one
// thread per channel vector that writes.
DEV void gn_store_groups(float* __restrict__ dst, const float (&s)[4],
                         const GnP& p, const GnT& t, bool w) {
  if (!(w && t.cok)) return;
  const int Cg = 1 << p.cgs;
  if (Cg >= 8) {
    if ((t.c0 & (Cg - 1)) == 0) dst[t.c0 >> p.cgs] = s[0];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (((2 * j) & (Cg - 1)) == 0) dst[(t.c0 + 2 * j) >> p.cgs] = s[j];
  }
}

DEV void gn_ld8(const float* __restrict__ p, float (&d)[8]) {
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
  d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
}

// γ, β of the lane's channels.  Scalar loads: the flat engine's parameter
// views are only 4-byte aligned.
DEV void gn_ld_param(const float* __restrict__ q, const GnT& t,
                     float (&d)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e++) d[e] = t.cok ? q[t.c0 + e] : 0.f;
}

// The row vector at element offset o: the bf16 tensor, or the sum of the f32
// slabs in slab order, rounded once and stored as the conv output.
template <bool F32SRC>
DEV V8 gn_load_src(const bf16* __restrict__ x, const float* __restrict__ slabs,
                   bf16* __restrict__ convout, long o, const GnP& p) {
  V8 v;
  if (!F32SRC) {
    v.u = *(const uint4*)(x + o);
    return v;
  }
  float f[8];
  gn_ld8(slabs + o, f);
  for (int sp = 1; sp < p.nsplit; sp++) {
    float g[8];
    gn_ld8(slabs + (long)sp * p.sstride + o, g);
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] += g[e];
  }
#pragma unroll
  for (int e = 0; e < 8; e++) v.e[e] = f2b(f[e]);
  *(uint4*)(convout + o) = v.u;
  return v;
}

// ----------------------------------------------------------------- forward --
// mean and M2 = Σ(x − mean)² of every group of the slab over rows [r0, r1),
// broadcast form.  base = element offset of (n, row 0, c0).
template <bool F32SRC>
DEV void gn_stats_rows(const bf16* __restrict__ x,
                       const float* __restrict__ slabs,
                       bf16* __restrict__ convout, long base, int r0, int r1,
                       const GnP& p, const GnT& t, uint4* rows, float* red,
                       float (&mean)[4], float (&m2)[4]) {
  const int Cg = 1 << p.cgs;
  const int iters = (r1 - r0 + t.rpp - 1) / t.rpp;  // block-uniform
  const bf16* src = F32SRC ? convout : x;
  float acc[8], s[4];
#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] = 0.f;
  for (int it = 0; it < iters; it++) {
    const int r = r0 + it * t.rpp + t.rr;
    V8 v;
    v.u = uint4{0, 0, 0, 0};
    if (t.cok && r < r1)
      v = gn_load_src<F32SRC>(x, slabs, convout, base + (long)r * p.C, p);
    if (it < p.resident) rows[it * GN_THREADS + t.tid] = v.u;
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] += b2f(v.e[e]);
  }
  gn_group_fold(acc, Cg, s);
  gn_block_sum<4>(s, t, p.lpr, red);
  const float inv = 1.f / (float)((r1 - r0) * Cg);
#pragma unroll
  for (int j = 0; j < 4; j++) mean[j] = s[j] * inv;

#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] = 0.f;
  for (int it = 0; it < iters; it++) {
    const int r = r0 + it * t.rpp + t.rr;
    const bool ok = t.cok && r < r1;
    V8 v;
    v.u = uint4{0, 0, 0, 0};
    if (it < p.resident)
      v.u = rows[it * GN_THREADS + t.tid];
    else if (ok)  // the thread's own store when F32SRC
      v.u = *(const uint4*)(src + base + (long)r * p.C);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float d = ok ? b2f(v.e[e]) - mean[e >> 1] : 0.f;
      acc[e] += d * d;
    }
  }
  gn_group_fold(acc, Cg, s);
  gn_block_sum<4>(s, t, p.lpr, red);
#pragma unroll
  for (int j = 0; j < 4; j++) m2[j] = s[j];
}

// y = act(a·x + b [+ residual]) over rows [r0, r1); a = γ·rstd, b = β − μ·a.
// No shuffle or barrier follows, so rows past the end are simply skipped.
template <int ACT>
DEV void gn_apply_rows(const bf16* __restrict__ src,
                       const bf16* __restrict__ res, bf16* __restrict__ y,
                       long base, int r0, int r1, int resident,
                       const float (&a)[8], const float (&b)[8],
                       const GnP& p, const GnT& t, const uint4* rows) {
  const int iters = (r1 - r0 + t.rpp - 1) / t.rpp;
  for (int it = 0; it < iters; it++) {
    const int r = r0 + it * t.rpp + t.rr;
    if (!(t.cok && r < r1)) continue;
    const long o = base + (long)r * p.C;
    V8 v, rv, out;
    if (it < resident)
      v.u = rows[it * GN_THREADS + t.tid];
    else
      v.u = *(const uint4*)(src + o);
    if (res) rv.u = *(const uint4*)(res + o);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float f = a[e] * b2f(v.e[e]) + b[e];
      if (res) f += b2f(rv.e[e]);
      if (ACT == 1) f = fmaxf(f, 0.f);
      else if (ACT == 2) f = fminf(fmaxf(f, 0.f), 6.f);
      out.e[e] = f2b(f);
    }
    *(uint4*)(y + o) = out.u;
  }
}

// a, b of the lane's channels from its groups' statistics.
DEV void gn_fold_affine(const float* __restrict__ gamma,
                        const float* __restrict__ beta, const GnT& t,
                        const float (&mean)[4], const float (&rstd)[4],
                        float (&a)[8], float (&b)[8]) {
  float gm[8], bt[8];
  gn_ld_param(gamma, t, gm);
  gn_ld_param(beta, t, bt);
#pragma unroll
  for (int e = 0; e < 8; e++) {
    a[e] = gm[e] * rstd[e >> 1];
    b[e] = bt[e] - mean[e >> 1] * a[e];
  }
}

// One launch: reduce, barrier, apply.  grid = (slabs, N).
template <bool F32SRC, int ACT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_fwd(
    const bf16* __restrict__ x, const float* __restrict__ slabs,
    bf16* __restrict__ convout, const bf16* __restrict__ res,
    bf16* __restrict__ y, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, GnP p) {
  extern __shared__ uint4 gn_rows[];
  __shared__ float red[4 * 8 * 64];
  const GnT t = gn_place(p);
  const int n = blockIdx.y;
  const long base = (long)n * p.HW * p.C + t.c0;
  float mean[4], m2[4], rstd[4], a[8], b[8];
  gn_stats_rows<F32SRC>(x, slabs, convout, base, 0, p.HW, p, t, gn_rows, red,
                        mean, m2);
  const float inv = 1.f / (float)(p.HW << p.cgs);
#pragma unroll
  for (int j = 0; j < 4; j++) rstd[j] = rsqrtf(m2[j] * inv + p.eps);
  gn_store_groups(mean_out + (long)n * p.G, mean, p, t, t.rr == 0);
  gn_store_groups(rstd_out + (long)n * p.G, rstd, p, t, t.rr == 0);
  gn_fold_affine(gamma, beta, t, mean, rstd, a, b);
  gn_apply_rows<ACT>(F32SRC ? convout : x, res, y, base, 0, p.HW, p.resident,
                     a, b, p, t, gn_rows);
}

// Split form, first launch: (mean, M2) of every group over the chunk
// blockIdx.z -> part[n][z][G][2].  grid = (slabs, N, Z).
template <bool F32SRC>
__global__ __launch_bounds__(GN_THREADS) void k_gn_stats_partial(
    const bf16* __restrict__ x, const float* __restrict__ slabs,
    bf16* __restrict__ convout, float* __restrict__ part, GnP p) {
  extern __shared__ uint4 gn_rows[];
  __shared__ float red[4 * 8 * 64];
  const GnT t = gn_place(p);
  const int n = blockIdx.y, z = blockIdx.z;
  const long base = (long)n * p.HW * p.C + t.c0;
  const int r0 = z * p.chunk, r1 = min(p.HW, r0 + p.chunk);
  float mean[4], m2[4];
  gn_stats_rows<F32SRC>(x, slabs, convout, base, r0, r1, p, t, gn_rows, red,
                        mean, m2);
  if (t.rr == 0 && t.cok) {
    float* pp = part + ((long)n * p.Z + z) * p.G * 2;
    const int Cg = 1 << p.cgs;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = t.c0 + 2 * j;
      if ((c & (Cg - 1)) == 0) {
        pp[(c >> p.cgs) * 2] = mean[j];
        pp[(c >> p.cgs) * 2 + 1] = m2[j];
      }
    }
  }
}

// Split form, second launch: every workgroup merges the chunks' pairs of its
// groups in chunk order (Chan), then applies to its own chunk.
template <int ACT>
__global__ __launch_bounds__(GN_THREADS) void k_gn_apply(
    const bf16* __restrict__ src, const float* __restrict__ part,
    const bf16* __restrict__ res, bf16* __restrict__ y,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, GnP p) {
  const GnT t = gn_place(p);
  const int n = blockIdx.y, z = blockIdx.z;
  const long base = (long)n * p.HW * p.C + t.c0;
  const float* pp = part + (long)n * p.Z * p.G * 2;
  int gi[4];
#pragma unroll
  for (int j = 0; j < 4; j++) gi[j] = t.cok ? (t.c0 + 2 * j) >> p.cgs : 0;
  float mean[4], m2[4], rstd[4], a[8], b[8];
  float cnt = 0.f;
  for (int zz = 0; zz < p.Z; zz++) {
    const float nb = (float)(min(p.chunk, p.HW - zz * p.chunk) << p.cgs);
    const float tot = cnt + nb;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float mb = pp[((long)zz * p.G + gi[j]) * 2];
      const float qb = pp[((long)zz * p.G + gi[j]) * 2 + 1];
      if (zz == 0) {
        mean[j] = mb;
        m2[j] = qb;
      } else {
        const float d = mb - mean[j];
        mean[j] += d * (nb / tot);
        m2[j] += qb + d * d * (cnt * (nb / tot));
      }
    }
    cnt = tot;
  }
#pragma unroll
  for (int j = 0; j < 4; j++) rstd[j] = rsqrtf(m2[j] / cnt + p.eps);
  gn_store_groups(mean_out + (long)n * p.G, mean, p, t, z == 0 && t.rr == 0);
  gn_store_groups(rstd_out + (long)n * p.G, rstd, p, t, z == 0 && t.rr == 0);
  gn_fold_affine(gamma, beta, t, mean, rstd, a, b);
  const int r0 = z * p.chunk, r1 = min(p.HW, r0 + p.chunk);
  gn_apply_rows<ACT>(src, res, y, base, r0, r1, 0, a, b, p, t, nullptr);
}

// ---------------------------------------------------------------- backward --
// g = dy where the activation passed: ReLU y > 0, ReLU6 0 < y < 6.
template <int MASK>
DEV V8 gn_mask(V8 d, const V8& yv) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const float f = b2f(yv.e[e]);
    if (MASK == 1 ? !(f > 0.f) : (MASK == 2 && (f <= 0.f || f >= 6.f)))
      d.e[e] = f2b(0.f);
  }
  return d;
}

DEV void gn_ld_stats(const float* __restrict__ q, const GnP& p, const GnT& t,
                     float (&d)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) d[j] = t.cok ? q[(t.c0 + 2 * j) >> p.cgs] : 0.f;
}

template <int MASK>
DEV void gn_ld_gx(const bf16* __restrict__ dy, const bf16* __restrict__ y,
                  const bf16* __restrict__ x, long o, V8& d, V8& xv) {
  d.u = *(const uint4*)(dy + o);
  if (MASK) {
    V8 yv;
    yv.u = *(const uint4*)(y + o);
    d = gn_mask<MASK>(d, yv);
  }
  xv.u = *(const uint4*)(x + o);
}

// Per-channel Σg and Σg·x̂ over rows [r0, r1), in every thread that holds
// the channels.  g and x stay in LDS for the first p.resident iterations.
template <int MASK>
DEV void gn_bwd_sums(const bf16* __restrict__ dy, const bf16* __restrict__ y,
                     const bf16* __restrict__ x, long base, int r0, int r1,
                     const float (&mu)[4], const float (&rs)[4],
                     const GnP& p, const GnT& t, uint4* rows, float* red,
                     float (&ag)[8], float (&agx)[8]) {
  const int iters = (r1 - r0 + t.rpp - 1) / t.rpp;
#pragma unroll
  for (int e = 0; e < 8; e++) ag[e] = agx[e] = 0.f;
  for (int it = 0; it < iters; it++) {
    const int r = r0 + it * t.rpp + t.rr;
    V8 d, xv;
    d.u = xv.u = uint4{0, 0, 0, 0};
    if (t.cok && r < r1)
      gn_ld_gx<MASK>(dy, y, x, base + (long)r * p.C, d, xv);
    if (it < p.resident) {
      rows[it * GN_THREADS + t.tid] = d.u;
      rows[(p.resident + it) * GN_THREADS + t.tid] = xv.u;
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const float g = b2f(d.e[e]);
      const float xh = (b2f(xv.e[e]) - mu[e >> 1]) * rs[e >> 1];
      ag[e] += g;
      agx[e] += g * xh;
    }
  }
  gn_block_sum<8>(ag, t, p.lpr, red);
  gn_block_sum<8>(agx, t, p.lpr, red);
}

// dconv and dres over rows [r0, r1) from the channel totals.
template <int MASK>
DEV void gn_bwd_rows(const bf16* __restrict__ dy, const bf16* __restrict__ y,
                     const bf16* __restrict__ x, bf16* __restrict__ dconv,
                     bf16* __restrict__ dres, const float* __restrict__ gamma,
                     long base, int r0, int r1, int resident,
                     const float (&mu)[4], const float (&rs)[4],
                     const float (&ag)[8], const float (&agx)[8],
                     const GnP& p, const GnT& t, const uint4* rows) {
  float gm[8], v1[8], v2[8], s1[4], s2[4];
  gn_ld_param(gamma, t, gm);
#pragma unroll
  for (int e = 0; e < 8; e++) {
    v1[e] = gm[e] * ag[e];
    v2[e] = gm[e] * agx[e];
  }
  gn_group_fold(v1, 1 << p.cgs, s1);
  gn_group_fold(v2, 1 << p.cgs, s2);
  const float inv = 1.f / (float)(p.HW << p.cgs);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    s1[j] *= inv;
    s2[j] *= inv;
  }
  const int iters = (r1 - r0 + t.rpp - 1) / t.rpp;
  for (int it = 0; it < iters; it++) {
    const int r = r0 + it * t.rpp + t.rr;
    if (!(t.cok && r < r1)) continue;
    const long o = base + (long)r * p.C;
    V8 d, xv, out;
    if (it < resident) {
      d.u = rows[it * GN_THREADS + t.tid];
      xv.u = rows[(resident + it) * GN_THREADS + t.tid];
    } else {
      gn_ld_gx<MASK>(dy, y, x, o, d, xv);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int j = e >> 1;
      const float xh = (b2f(xv.e[e]) - mu[j]) * rs[j];
      out.e[e] = f2b(rs[j] * (b2f(d.e[e]) * gm[e] - (s1[j] + xh * s2[j])));
    }
    *(uint4*)(dconv + o) = out.u;
    if (dres) *(uint4*)(dres + o) = d.u;
  }
}

// (Σg, Σg·x̂) of the lane's 8 channels, interleaved as [C][2].
DEV void gn_st_pairs(float* __restrict__ q, const float (&ag)[8],
                     const float (&agx)[8]) {
#pragma unroll
  for (int k = 0; k < 4; k++)
    *(float4*)(q + 4 * k) =
        float4{ag[2 * k], agx[2 * k], ag[2 * k + 1], agx[2 * k + 1]};
}

// One launch per (sample, slab): sums, barrier, apply; the channel totals of
// the sample go to ws[n][C][2].  grid = (slabs, N).
template <int MASK>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd(
    const bf16* __restrict__ dy, const bf16* __restrict__ y,
    const bf16* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    bf16* __restrict__ dconv, bf16* __restrict__ dres,
    float* __restrict__ ws, GnP p) {
  extern __shared__ uint4 gn_rows[];
  __shared__ float red[4 * 8 * 64];
  const GnT t = gn_place(p);
  const int n = blockIdx.y;
  const long base = (long)n * p.HW * p.C + t.c0;
  float mu[4], rs[4], ag[8], agx[8];
  gn_ld_stats(mean + (long)n * p.G, p, t, mu);
  gn_ld_stats(rstd + (long)n * p.G, p, t, rs);
  gn_bwd_sums<MASK>(dy, y, x, base, 0, p.HW, mu, rs, p, t, gn_rows, red, ag,
                    agx);
  if (t.rr == 0 && t.cok)
    gn_st_pairs(ws + ((long)n * p.C + t.c0) * 2, ag, agx);
  gn_bwd_rows<MASK>(dy, y, x, dconv, dres, gamma, base, 0, p.HW, p.resident,
                    mu, rs, ag, agx, p, t, gn_rows);
}

// Split form, first launch: the chunk's channel sums -> part[n][z][C][2].
template <int MASK>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_partial(
    const bf16* __restrict__ dy, const bf16* __restrict__ y,
    const bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, float* __restrict__ part, GnP p) {
  extern __shared__ uint4 gn_rows[];
  __shared__ float red[4 * 8 * 64];
  const GnT t = gn_place(p);
  const int n = blockIdx.y, z = blockIdx.z;
  const long base = (long)n * p.HW * p.C + t.c0;
  const int r0 = z * p.chunk, r1 = min(p.HW, r0 + p.chunk);
  float mu[4], rs[4], ag[8], agx[8];
  gn_ld_stats(mean + (long)n * p.G, p, t, mu);
  gn_ld_stats(rstd + (long)n * p.G, p, t, rs);
  gn_bwd_sums<MASK>(dy, y, x, base, r0, r1, mu, rs, p, t, gn_rows, red, ag,
                    agx);
  if (t.rr == 0 && t.cok)
    gn_st_pairs(part + (((long)n * p.Z + z) * p.C + t.c0) * 2, ag, agx);
}

// Split form, second launch: the chunks' sums in chunk order, then the apply
// on the workgroup's own chunk; chunk 0 also emits the sample's totals.
template <int MASK>
__global__ __launch_bounds__(GN_THREADS) void k_gn_bwd_apply(
    const bf16* __restrict__ dy, const bf16* __restrict__ y,
    const bf16* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ part, bf16* __restrict__ dconv,
    bf16* __restrict__ dres, float* __restrict__ ws, GnP p) {
  const GnT t = gn_place(p);
  const int n = blockIdx.y, z = blockIdx.z;
  const long base = (long)n * p.HW * p.C + t.c0;
  float mu[4], rs[4], ag[8], agx[8];
  gn_ld_stats(mean + (long)n * p.G, p, t, mu);
  gn_ld_stats(rstd + (long)n * p.G, p, t, rs);
#pragma unroll
  for (int e = 0; e < 8; e++) ag[e] = agx[e] = 0.f;
  if (t.cok) {
    for (int zz = 0; zz < p.Z; zz++) {
      const float* q = part + (((long)n * p.Z + zz) * p.C + t.c0) * 2;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const float4 v = *(const float4*)(q + 4 * k);
        ag[2 * k] += v.x;
        agx[2 * k] += v.y;
        ag[2 * k + 1] += v.z;
        agx[2 * k + 1] += v.w;
      }
    }
  }
  if (z == 0 && t.rr == 0 && t.cok)
    gn_st_pairs(ws + ((long)n * p.C + t.c0) * 2, ag, agx);
  const int r0 = z * p.chunk, r1 = min(p.HW, r0 + p.chunk);
  gn_bwd_rows<MASK>(dy, y, x, dconv, dres, gamma, base, r0, r1, 0, mu, rs, ag,
                    agx, p, t, nullptr);
}

// dβ[c] (+)= Σ_n ws[n][c][0], dγ[c] (+)= Σ_n ws[n][c][1], n ascending.
__global__ __launch_bounds__(GN_THREADS) void k_gn_param_reduce(
    const float* __restrict__ ws, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int N, int C, int accum) {
  const int c = blockIdx.x * GN_THREADS + threadIdx.x;
  if (c >= C) return;
  float sb = 0.f, sg = 0.f;
  for (int n = 0; n < N; n++) {
    const float2 v = *(const float2*)(ws + ((long)n * C + c) * 2);
    sb += v.x;
    sg += v.y;
  }
  dbeta[c] = accum ? dbeta[c] + sb : sb;
  dgamma[c] = accum ? dgamma[c] + sg : sg;
}

// -------------------------------------------------------------- launchers --
static long g_gn_fwd = 0, g_gn_bwd = 0;
// Rows per sample above which the split form runs (docs/TUNING.md).
static long g_gn_split_hw = env_long("HZ_GN_SPLIT_HW", 512);

// Lanes per row.  8 lanes (64 channels, one full 128-byte line) hold whole
// groups for every served Cg; the slab widens while a pass of 256/lpr rows
// would be longer than the sample and C has the channels.  Reads C, Cg and
// HW only: a sample's reduction order must not depend on the batch.
static int gn_pick_lpr(int C, int Cg, int HW) {
  int lpr = std::max(8, Cg / 8);
  const int cpad = (C + 63) / 64 * 64;
  while (lpr < 64 && 16 * lpr <= cpad && GN_THREADS / lpr > HW) lpr *= 2;
  return lpr;
}

static GnP gn_geometry(int HW, int C, int G, int bwd) {
  GnP p{};
  p.HW = HW;
  p.C = C;
  p.G = G;
  const int Cg = C / G;
  while ((1 << p.cgs) < Cg) p.cgs++;
  p.lpr = gn_pick_lpr(C, Cg, HW);
  const int rpp = GN_THREADS / p.lpr;
  const int cap = bwd ? GN_RES_ITERS / 2 : GN_RES_ITERS;
  long chunk = HW;
  if (HW > g_gn_split_hw) {
    // a chunk stays resident; no more chunks than a grid axis takes
    chunk = std::min(g_gn_split_hw, (long)cap * rpp);
    chunk = std::max(chunk, (long)(HW + 65534) / 65535);
  }
  p.chunk = (int)chunk;
  p.Z = (HW + p.chunk - 1) / p.chunk;
  p.resident = std::min((p.chunk + rpp - 1) / rpp, cap);
  return p;
}

template <class F>
static void gn_with_act(int act, F&& f) {
  if (act == 1) f(std::integral_constant<int, 1>{});
  else if (act == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 0>{});
}

extern "C" {

void set_gn_split_hw(long rows) { g_gn_split_hw = std::max(1L, rows); }
long gn_split_hw() { return g_gn_split_hw; }

int gn_splits(int HW, int C, int G, int bwd) {
  return gn_geometry(HW, C, G, bwd).Z;
}

void gn_launch_counts(long* fwd, long* bwd) {
  *fwd = g_gn_fwd;
  *bwd = g_gn_bwd;
}

void launch_gn_fwd(const void* x, const float* slabs, int nsplit,
                   void* convout, const void* res, void* y,
                   const float* gamma, const float* beta, float* mean,
                   float* rstd, float* part, int N, int HW, int C, int G,
                   float eps, int act, hipStream_t st) {
  GnP p = gn_geometry(HW, C, G, 0);
  p.eps = eps;
  p.nsplit = nsplit;
  p.sstride = (long)N * HW * C;
  const int nslab = (C + 8 * p.lpr - 1) / (8 * p.lpr);
  const size_t lds = (size_t)p.resident * GN_THREADS * 16;
  const bf16 *xp = (const bf16*)x, *rp = (const bf16*)res;
  bf16 *cp = (bf16*)convout, *yp = (bf16*)y;
  const bf16* src = slabs ? cp : xp;
  if (p.Z == 1) {
    const dim3 grid(nslab, N);
    gn_with_act(act, [&](auto a) {
      if (slabs)
        k_gn_fwd<true, decltype(a)::value><<<grid, GN_THREADS, lds, st>>>(
            xp, slabs, cp, rp, yp, gamma, beta, mean, rstd, p);
      else
        k_gn_fwd<false, decltype(a)::value><<<grid, GN_THREADS, lds, st>>>(
            xp, slabs, cp, rp, yp, gamma, beta, mean, rstd, p);
    });
    g_gn_fwd += 1;
    return;
  }
  const dim3 grid(nslab, N, p.Z);
  if (slabs)
    k_gn_stats_partial<true><<<grid, GN_THREADS, lds, st>>>(xp, slabs, cp,
                                                            part, p);
  else
    k_gn_stats_partial<false><<<grid, GN_THREADS, lds, st>>>(xp, slabs, cp,
                                                             part, p);
  gn_with_act(act, [&](auto a) {
    k_gn_apply<decltype(a)::value><<<grid, GN_THREADS, 0, st>>>(src, part, rp, yp, gamma,
                                                     beta, mean, rstd, p);
  });
  g_gn_fwd += 2;
}

void launch_gn_bwd(const void* dy, const void* y, const void* x,
                   const float* gamma, const float* mean, const float* rstd,
                   void* dconv, void* dres, float* ws, float* part,
                   float* dgamma, float* dbeta, int accum, int N, int HW,
                   int C, int G, int act, hipStream_t st) {
  const GnP p = gn_geometry(HW, C, G, 1);
  const int nslab = (C + 8 * p.lpr - 1) / (8 * p.lpr);
  const size_t lds = (size_t)p.resident * 2 * GN_THREADS * 16;
  const bf16 *dyp = (const bf16*)dy, *yp = (const bf16*)y,
             *xp = (const bf16*)x;
  bf16 *dcp = (bf16*)dconv, *drp = (bf16*)dres;
  if (p.Z == 1) {
    gn_with_act(act, [&](auto m) {
      k_gn_bwd<decltype(m)::value><<<dim3(nslab, N), GN_THREADS, lds, st>>>(
          dyp, yp, xp, gamma, mean, rstd, dcp, drp, ws, p);
    });
    g_gn_bwd += 2;
  } else {
    const dim3 grid(nslab, N, p.Z);
    gn_with_act(act, [&](auto m) {
      k_gn_bwd_partial<decltype(m)::value><<<grid, GN_THREADS, lds, st>>>(
          dyp, yp, xp, mean, rstd, part, p);
      k_gn_bwd_apply<decltype(m)::value><<<grid, GN_THREADS, 0, st>>>(
          dyp, yp, xp, gamma, mean, rstd, part, dcp, drp, ws, p);
    });
    g_gn_bwd += 3;
  }
  k_gn_param_reduce<<<(C + GN_THREADS - 1) / GN_THREADS, GN_THREADS, 0, st>>>(
      ws, dgamma, dbeta, N, C, accum);
}

}  // extern "C"
