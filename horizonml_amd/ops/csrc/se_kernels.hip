// Squeeze-and-Excitation for gfx950 (MI355X, CDNA4).  docs/KERNELS.md,
// "Squeeze-and-Excitation".
//
//   s[n,c] = mean_hw u[n,hw,c]                       k_se_pool<0>  (squeeze)
//   h[n,j] = relu(W1·s + b1), g[n,c] = σ(W2·h + b2)  k_se_excite
//   y      = act(u·g + residual)                     k_se_scale
// and backward
//   dg[n,c] = Σ_hw dz·u, dz = dy·(y > 0)             k_se_pool<1|2>
//   da2 = dg·g·(1−g); dW2, db2, dh                   k_se_excite_bwd<true>
//   dW1, db1, ds                                     k_se_excite_bwd<false>
//   du = dz·g + ds/HW, dres = dz                     k_se_bwd_apply
//
// u, residual, y, dy, du, dres are bf16 NHWC; s, h, g and every gradient of
// the MLP are f32; W1 [Cr,C] and W2 [C,Cr] are the bf16 shadows.  Served
// range (checked in bind.cpp): C % 8 == 0, C ≤ 2048, 4 ≤ Cr ≤ 128,
// Cr % 4 == 0.  No kernel here has an atomic: every cross-lane, cross-wave
// and cross-block sum runs in a fixed order, so default and deterministic
// mode run the same code and two runs agree bitwise.
//
// Streaming kernels: a lane owns 8 adjacent channels (one 16-byte access per
// pixel), L = C/8 lanes cover a pixel.  MFMA fragment maps are the ones at
// the top of head_kernels.hip (lane = (r = lane & 15, g = lane >> 4)).  The
// f32 operands of the MLP (s, h, da2, dh) enter the bf16 matrix unit as the
// three-term split of k_head_bwd, smallest term first, so the MLP keeps f32
// numerics; where both operands are f32 all nine term products are issued.
//
// EXEC rule (docs/KERNELS.md): transposed reads and MFMAs run with EXEC all
// ones.  Roles, tiles and loop bounds are block- or wave-uniform; rows ≥ N,
// columns ≥ C / Cr are ZEROS in fragments and images, never masked lanes and
// never read out of bounds.
#include "common.h"

#include <algorithm>

// ------------------------------------------------ small shared device code --
// se_split3 / se_read_tr_frag are k_head_bwd's helpers (head_kernels.hip
// keeps its own copies; that file is left as it is).
DEV void se_split3(const float (&d)[8], V8& hi, V8& mid, V8& lo) {
#pragma clang fp reassociate(off)
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const bf16 h = f2b(d[e]);
    const float r1 = d[e] - b2f(h);
    const bf16 m = f2b(r1);
    const float r2 = r1 - b2f(m);
    hi.e[e] = h;
    mid.e[e] = m;
    lo.e[e] = f2b(r2);
  }
}

DEV bf16x8 se_read_tr_frag(const bf16* img, int off) {
  const bf16x4 lo = lds_read_tr16(img + off);
  const bf16x4 hi = lds_read_tr16(img + off + 4 * 64);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

DEV f32x4 se_mfma(const V8& a, const V8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}

DEV void se_ld8(const float* p, float (&d)[8]) {
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
  d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
}

DEV void se_st8(float* p, const float (&d)[8]) {
  *(float4*)p = float4{d[0], d[1], d[2], d[3]};
  *(float4*)(p + 4) = float4{d[4], d[5], d[6], d[7]};
}

// m[n][col .. col+7] of an f32 [N][ld] matrix, zeros past N / ld.  ld % 4
// == 0, col % 8 == 0 and a 16-byte aligned base make the rows float4-aligned.
DEV void se_load8(const float* __restrict__ m, int N, int ld, int n, int col,
                  float (&d)[8]) {
  const float* p = m + (long)n * ld + col;
  if (n < N && col + 8 <= ld) {
    se_ld8(p, d);
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++) d[e] = (n < N && col + e < ld) ? p[e] : 0.f;
  }
}

// Σ over the H·W splits, in split order, of part[n][sp][col .. col+7].
DEV void se_fold8(const float* __restrict__ part, int splits, int C, int n,
                  int col, float (&d)[8]) {
  const float* p = part + (long)n * splits * C + col;
  se_ld8(p, d);
  for (int sp = 1; sp < splits; sp++) {
    float t[8];
    se_ld8(p + (long)sp * C, t);
#pragma unroll
    for (int e = 0; e < 8; e++) d[e] += t[e];
  }
}

// w[row][col .. col+7] of a bf16 [rows][ld] matrix, zeros past rows / ld.
// ld % 4 == 0 only (Cr = 4 is an 8-byte row), so two 8-byte halves.
DEV V8 se_load_w8(const bf16* __restrict__ w, int rows, int ld, int row,
                  int col) {
  union { V8 v; uint2 h[2]; } t;
  t.v.u = uint4{0, 0, 0, 0};
  if (row < rows) {
    const bf16* p = w + (long)row * ld + col;
    if (col + 4 <= ld) t.h[0] = *(const uint2*)p;
    if (col + 8 <= ld) t.h[1] = *(const uint2*)(p + 4);
  }
  return t.v;
}

// ------------------------------------------------------ squeeze / dg reduce --
// part[n][sp][c] f32 = Σ over the pixels of split sp of
//   MODE 0: u      MODE 1: dy·u      MODE 2: dy·(y > 0)·u
//   grid    (N, splits); split sp owns pixels [sp·chunk, (sp+1)·chunk)
//   narrow  (L ≤ 64) a wave walks 64/L pixels per load and the four waves
//           interleave; lanes holding the same channels are folded into the
//           wave's first pixel row with cross-lane moves, pixel row 1, 2, ...
//           in order, then the waves through LDS in wave order
//   wide    (L > 64) the block walks 256/L (1..3) pixels per load, folded
//           through LDS in pixel-row order
// Either way at most 2048 floats of LDS: 4·C with C ≤ 512, or (256/L)·C.
template <int MODE>
__global__ __launch_bounds__(256) void k_se_pool(
    const bf16* __restrict__ u, const bf16* __restrict__ dy,
    const bf16* __restrict__ y, float* __restrict__ part, int HW, int C,
    int chunk) {
  __shared__ float fold[2048];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = C >> 3;
  const bool narrow = L <= 64;  // block-uniform
  const int ppg = (narrow ? 64 : 256) / L;
  const int t = narrow ? lane : tid;
  const int cl = t % L, pp = t / L;
  const bool live = pp < ppg;
  const int first = narrow ? wave * ppg + pp : pp;
  const int stride = narrow ? 4 * ppg : ppg;
  const int n = blockIdx.x, sp = blockIdx.y;
  const int p0 = sp * chunk, p1 = min(HW, p0 + chunk);
  const long base = (long)n * HW * C + cl * 8;

  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; e++) acc[e] = 0.f;
  if (live) {
#pragma unroll 4
    for (int p = p0 + first; p < p1; p += stride) {
      const long o = base + (long)p * C;
      V8 a, b, c;
      a.u = *(const uint4*)(u + o);
      if (MODE >= 1) b.u = *(const uint4*)(dy + o);
      if (MODE == 2) c.u = *(const uint4*)(y + o);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float v = b2f(a.e[e]);
        if (MODE >= 1) v *= b2f(b.e[e]);
        if (MODE == 2) v = b2f(c.e[e]) > 0.f ? v : 0.f;
        acc[e] += v;
      }
    }
  }
  if (narrow) {
    // every lane runs the moves; only a wave's first pixel row keeps the sum
    for (int j = 1; j < ppg; j++) {
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float o = __shfl(acc[e], cl + j * L, 64);
        if (pp == 0) acc[e] += o;
      }
    }
  }
  const int slot = narrow ? wave : pp;
  const int nslot = narrow ? 4 : ppg;
  if (narrow ? pp == 0 : live) {
#pragma unroll
    for (int e = 0; e < 8; e++) fold[slot * C + cl * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < L) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = fold[tid * 8 + e];
    for (int k = 1; k < nslot; k++) {
#pragma unroll
      for (int e = 0; e < 8; e++) v[e] += fold[k * C + tid * 8 + e];
    }
    se_st8(part + ((long)n * gridDim.y + sp) * C + tid * 8, v);
  }
}

// ------------------------------------------------------------------ excite --
// One launch for fold + FC1 + ReLU + FC2 + sigmoid, the batch as the MFMA M
// dimension.
//   block   16 images × 64 gate columns; grid = (ceil(C/64), ceil(N/16))
//   FC1     h[16][Cr] over the WHOLE of Cr, recomputed by every column tile
//           (16·C·Cr MACs, cheaper than a launch boundary).  K = C is split
//           over the four waves in 32-k steps, wave w takes steps w, w+4, …
//           A fragment: lane (r, g) folds the squeeze partials of image r,
//           channels k0+8g..+7, in split order, scales by 1/HW (that IS s,
//           stored by column tile 0) and splits it in three.  B fragment: a
//           W1[j = 16·jt + r][k0+8g..+7] in two 8-byte loads, K-major as it
//           lies.
//           The four partial tiles meet in LDS and are summed in wave order,
//           then bias and ReLU; h stays in LDS (column tile 0 stores it).
//   FC2     wave w owns gate columns c0+16w..+15, K = Cr in 32-steps from
//           the LDS h (three-term split again), B from W2[c][j..] K-major.
// Rounding chain: s ≤ splits adds + 1 scale; h ≤ C/128 MFMA steps of 32
// products, 3 combines, 1 bias; g ≤ Cr/32 steps, 1 bias, the sigmoid.
__global__ __launch_bounds__(256) void k_se_excite(
    const float* __restrict__ part, const bf16* __restrict__ w1,
    const float* __restrict__ b1, const bf16* __restrict__ w2,
    const float* __restrict__ b2, float* __restrict__ s,
    float* __restrict__ h, float* __restrict__ gate, int N, int C, int Cr,
    int splits, float inv_hw) {
  __shared__ float red[4][8 * 256];  // [wave][jt][q][lane]
  __shared__ __attribute__((aligned(16))) float hs[16][132];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int c0 = blockIdx.x * 64, m0 = blockIdx.y * 16;
  const int njt = (Cr + 15) >> 4;   // ≤ 8, block-uniform
  const int nk2 = (Cr + 31) >> 5;   // ≤ 4
  const int nks = (C + 31) >> 5;
  const int row = m0 + r;

  f32x4 acc[8] = {};
  for (int ks = wave; ks < nks; ks += 4) {
    const int k = ks * 32 + g * 8;
    const bool kok = k < C;  // C % 8 == 0: a lane's 8 k are all in or all out
    float sv[8];
#pragma unroll
    for (int e = 0; e < 8; e++) sv[e] = 0.f;
    if (row < N && kok) {
      se_fold8(part, splits, C, row, k, sv);
#pragma unroll
      for (int e = 0; e < 8; e++) sv[e] *= inv_hw;
      if (blockIdx.x == 0) se_st8(s + (long)row * C + k, sv);
    }
    V8 hi, mid, lo;
    se_split3(sv, hi, mid, lo);
#pragma unroll
    for (int jt = 0; jt < 8; jt++)
      if (jt < njt) {
        const int j = jt * 16 + r;
        // two 8-byte halves: the engine's shadow slices are only that aligned
        const V8 wf = se_load_w8(w1, Cr, C, j, k);
        acc[jt] = se_mfma(lo, wf, acc[jt]);
        acc[jt] = se_mfma(mid, wf, acc[jt]);
        acc[jt] = se_mfma(hi, wf, acc[jt]);
      }
  }
#pragma unroll
  for (int jt = 0; jt < 8; jt++)
    if (jt < njt) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        red[wave][(jt * 4 + q) * 64 + lane] = acc[jt][q];
    }
  __syncthreads();
  // h tile, zero-filled up to the 32-k steps FC2 reads
  for (int e = tid; e < nk2 * 2 * 256; e += 256) {
    const int jt = e >> 8, q = (e >> 6) & 3, ln = e & 63;
    const int hr = (ln >> 4) * 4 + q, j = jt * 16 + (ln & 15);
    float v = 0.f;
    if (jt < njt && j < Cr) {
      v = red[0][e];
      v += red[1][e];
      v += red[2][e];
      v += red[3][e];
      v = fmaxf(v + b1[j], 0.f);
      if (blockIdx.x == 0 && m0 + hr < N) h[(long)(m0 + hr) * Cr + j] = v;
    }
    hs[hr][j] = v;
  }
  __syncthreads();

  const int cc = c0 + wave * 16 + r;
  f32x4 o = {};
  for (int k2 = 0; k2 < nk2; k2++) {
    const int j = k2 * 32 + g * 8;
    float hv[8];
    se_ld8(&hs[r][j], hv);
    V8 hi, mid, lo;
    se_split3(hv, hi, mid, lo);
    const V8 wf = se_load_w8(w2, C, Cr, cc, j);
    o = se_mfma(lo, wf, o);
    o = se_mfma(mid, wf, o);
    o = se_mfma(hi, wf, o);
  }
  if (cc < C) {
    const float bias = b2[cc];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int n = m0 + g * 4 + q;
      if (n < N)
        gate[(long)n * C + cc] = 1.f / (1.f + __expf(-(o[q] + bias)));
    }
  }
}

// ------------------------------------------------------------------- scale --
// y = act(u·g[n,c] + residual).  grid = (pixel chunks, N); thread (pp, cl) of
// a block walks pixels pp, pp + 256/L, ... of its chunk with the gate of its
// 8 channels in registers.  No barrier, so the spare threads leave at once.
constexpr int SE_PIX_ITERS = 8;  // pixels per thread of k_se_scale / bwd_apply

template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void k_se_scale(
    const bf16* __restrict__ u, const float* __restrict__ gate,
    const bf16* __restrict__ res, bf16* __restrict__ y, int HW, int C) {
  const int tid = threadIdx.x;
  const int L = C >> 3, ppb = 256 / L;
  const int cl = tid % L, pp = tid / L;
  if (pp >= ppb) return;
  const int n = blockIdx.y;
  float gv[8];
  se_ld8(gate + (long)n * C + cl * 8, gv);
  const long base = (long)n * HW * C + cl * 8;
  const int p0 = blockIdx.x * (ppb * SE_PIX_ITERS) + pp;
#pragma unroll 4
  for (int it = 0; it < SE_PIX_ITERS; it++) {
    const int p = p0 + it * ppb;
    if (p >= HW) break;
    const long o = base + (long)p * C;
    V8 a, b, out;
    a.u = *(const uint4*)(u + o);
    if (RES) b.u = *(const uint4*)(res + o);
#pragma unroll
    for (int e = 0; e < 8; e++) {
      float v = b2f(a.e[e]) * gv[e];
      if (RES) v += b2f(b.e[e]);
      if (RELU) v = fmaxf(v, 0.f);
      out.e[e] = f2b(v);
    }
    *(uint4*)(y + o) = out.u;
  }
}

// du = dz·g + ds/HW, dres = dz (bitwise the masked dy), one pass; du does
// not depend on u.
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void k_se_bwd_apply(
    const bf16* __restrict__ dy, const bf16* __restrict__ y,
    const float* __restrict__ gate, const float* __restrict__ ds,
    bf16* __restrict__ du,
    bf16* __restrict__ dres, int HW, int C, float inv_hw) {
  const int tid = threadIdx.x;
  const int L = C >> 3, ppb = 256 / L;
  const int cl = tid % L, pp = tid / L;
  if (pp >= ppb) return;
  const int n = blockIdx.y;
  float gv[8], sv[8];
  se_ld8(gate + (long)n * C + cl * 8, gv);
  se_ld8(ds + (long)n * C + cl * 8, sv);
#pragma unroll
  for (int e = 0; e < 8; e++) sv[e] *= inv_hw;
  const long base = (long)n * HW * C + cl * 8;
  const int p0 = blockIdx.x * (ppb * SE_PIX_ITERS) + pp;
#pragma unroll 4
  for (int it = 0; it < SE_PIX_ITERS; it++) {
    const int p = p0 + it * ppb;
    if (p >= HW) break;
    const long o = base + (long)p * C;
    V8 d, m, out;
    d.u = *(const uint4*)(dy + o);
    if (RELU) {
      m.u = *(const uint4*)(y + o);
#pragma unroll
      for (int e = 0; e < 8; e++)
        if (!(b2f(m.e[e]) > 0.f)) d.e[e] = f2b(0.f);
    }
#pragma unroll
    for (int e = 0; e < 8; e++) out.e[e] = f2b(b2f(d.e[e]) * gv[e] + sv[e]);
    *(uint4*)(du + o) = out.u;
    if (RES) *(uint4*)(dres + o) = d.u;
  }
}

// --------------------------------------------------------- excite backward --
// Two launches of one kernel template; the boundary between them is the one
// true dependency (all of dh before any of dW1 / ds).
//   STAGE A  P = da2[n][c] = dg·g·(1−g), dg folded from the reduce partials
//            rowmat: dh[N][Cr]  = (P · W2)·(h > 0)     K = C
//            outer:  dW2[C][Cr] (+)= Pᵀ · h, db2 (+)= Σ_n P
//   STAGE B  P = dh[n][j]
//            rowmat: ds[N][C]   = P · W1               K = Cr
//            outer:  dW1[Cr][C] (+)= Pᵀ · s, db1 (+)= Σ_n P
// A block's role and tile come from blockIdx.x (block-uniform); every output
// element belongs to exactly one block, so nothing is added across blocks.
struct SeBwdArgs {
  const float* part;  // A: dg partials [N][splits][C]
  const float* gate;  // A: g [N][C]
  const float* p;     // B: dh [N][Cr]
  const float* q;     // outer's second operand: h (A) or s (B), [N][QC]
  const bf16* w;      // rowmat's weight [PC][QC]: W2 (A) or W1 (B)
  const float* mask;  // A: h, dh is zeroed where h == 0; B: nullptr
  float* out;         // rowmat output [N][QC]
  float* dw;          // [PC][QC]
  float* db;          // [PC]
  int N, PC, QC;      // batch, columns of P, columns of Q / W
  int splits, accum, dwvec;
  int nrow, ntq;      // rowmat blocks, ceil(QC / 64)
};

template <bool A>
DEV void se_load_p(const SeBwdArgs& a, int n, int col, float (&d)[8]) {
  if (A) {
    // PC = C, C % 8 == 0: the 8 columns are all inside or all outside
    if (n < a.N && col < a.PC) {
      float gv[8];
      se_fold8(a.part, a.splits, a.PC, n, col, d);
      se_ld8(a.gate + (long)n * a.PC + col, gv);
#pragma unroll
      for (int e = 0; e < 8; e++) d[e] = d[e] * gv[e] * (1.f - gv[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) d[e] = 0.f;
    }
  } else {
    se_load8(a.p, a.N, a.PC, n, col, d);
  }
}

union SeBwdSmem {
  struct {  // outer: [32 n][64] images of lds_tr_off<64>, lo / mid / hi
    __attribute__((aligned(16))) bf16 P[3][32 * 64];
    __attribute__((aligned(16))) bf16 Q[3][32 * 64];
  } o;
  __attribute__((aligned(16))) bf16 W[32 * 64];  // rowmat: [32 k][64 t]
  float out[64][65];  // outer epilogue: [P column][Q column]
  float dbp[32][64];  // db partials: [tile row][P column]
};

// rowmat: 64 batch rows × 64 output columns, reduction over PC in steps of
// 32 (head_dx_tile's form).  W[k][t] is reduction-rows × output-columns, so
// it is staged as it lies and read transposed; P[n][k..] is contiguous along
// the reduction: 8 f32 per lane, split in registers, are the A fragments.
template <bool A>
DEV void se_rowmat_tile(const SeBwdArgs& a, int m0, int t0, SeBwdSmem& smem) {
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // W tile: k row, 8-wide t
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
  int boff[2];
#pragma unroll
  for (int ni = 0; ni < 2; ni++)
    boff[ni] = lds_tr_off<64>(fk * 8 + (fr >> 2),
                              wc * 32 + ni * 16 + (fr & 3) * 4);
  float a_nx[2][8];
  V8 w_nx;
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
      se_load_p<A>(a, m0 + wr * 32 + mi * 16 + fr, k0 + fk * 8, a_nx[mi]);
    w_nx = se_load_w8(a.w, a.PC, a.QC, k0 + sm, t0 + sv);
  };

  f32x4 acc[2][2] = {};
  load_tile(0);
  for (int k0 = 0; k0 < a.PC; k0 += 32) {
    *(V8*)&smem.W[lds_tr_off<64>(sm, sv)] = w_nx;
    V8 af[3][2];  // lo, mid, hi
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
      se_split3(a_nx[mi], af[2][mi], af[1][mi], af[0][mi]);
    __syncthreads();
    if (k0 + 32 < a.PC) load_tile(k0 + 32);
    V8 bf[2];
#pragma unroll
    for (int ni = 0; ni < 2; ni++)
      bf[ni].v = se_read_tr_frag(smem.W, boff[ni]);
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int ni = 0; ni < 2; ni++)
          acc[mi][ni] = se_mfma(af[s][mi], bf[ni], acc[mi][ni]);
    __syncthreads();
  }
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      const int t = t0 + wc * 32 + ni * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int n = m0 + wr * 32 + mi * 16 + fk * 4 + q;
        if (n < a.N && t < a.QC) {
          const long o = (long)n * a.QC + t;
          float v = acc[mi][ni][q];
          if (A) v = a.mask[o] > 0.f ? v : 0.f;
          a.out[o] = v;
        }
      }
    }
}

// outer: 64 P columns × 64 Q columns, reduction over the batch in steps of
// 32 (head_dw_tile's form, with BOTH operands f32).  P[n][·] and Q[n][·] are
// reduction-rows × output-columns: one 16-byte LDS store per vec8 and term
// into lds_tr_off<64> images, fragments by two transposed reads, the nine
// term products smallest first.  Blocks of Q tile 0 also sum their 64 P
// columns over the batch: per tile row first, then the 32 tile rows in order.
template <bool A>
DEV void se_outer_tile(const SeBwdArgs& a, int j0, int t0, SeBwdSmem& smem) {
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // tile row n, 8-wide column
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
  int aoff[2], boff[2];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    aoff[i] = lds_tr_off<64>(fk * 8 + (fr >> 2),
                             wr * 32 + i * 16 + (fr & 3) * 4);
    boff[i] = lds_tr_off<64>(fk * 8 + (fr >> 2),
                             wc * 32 + i * 16 + (fr & 3) * 4);
  }
  float p_nx[8], q_nx[8], dbs[8];
  auto load_tile = [&](int n0) {
    se_load_p<A>(a, n0 + sm, j0 + sv, p_nx);
    se_load8(a.q, a.N, a.QC, n0 + sm, t0 + sv, q_nx);
  };
#pragma unroll
  for (int e = 0; e < 8; e++) dbs[e] = 0.f;

  f32x4 acc[2][2] = {};
  const int soff = lds_tr_off<64>(sm, sv);
  load_tile(0);
  for (int n0 = 0; n0 < a.N; n0 += 32) {
    V8 t[3];
    se_split3(p_nx, t[2], t[1], t[0]);
#pragma unroll
    for (int s = 0; s < 3; s++) *(V8*)&smem.o.P[s][soff] = t[s];
    se_split3(q_nx, t[2], t[1], t[0]);
#pragma unroll
    for (int s = 0; s < 3; s++) *(V8*)&smem.o.Q[s][soff] = t[s];
#pragma unroll
    for (int e = 0; e < 8; e++) dbs[e] += p_nx[e];
    __syncthreads();
    if (n0 + 32 < a.N) load_tile(n0 + 32);
    V8 af[3][2], bf[3][2];
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
      for (int i = 0; i < 2; i++) {
        af[s][i].v = se_read_tr_frag(smem.o.P[s], aoff[i]);
        bf[s][i].v = se_read_tr_frag(smem.o.Q[s], boff[i]);
      }
    // term pairs by magnitude: lo·lo first, hi·hi last
#pragma unroll
    for (int sum = 0; sum <= 4; sum++)
#pragma unroll
      for (int sa = 0; sa < 3; sa++) {
        const int sb = sum - sa;
        if (sb < 0 || sb > 2) continue;
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
          for (int ni = 0; ni < 2; ni++)
            acc[mi][ni] = se_mfma(af[sa][mi], bf[sb][ni], acc[mi][ni]);
      }
    __syncthreads();
  }

  if (t0 == 0) {  // block-uniform
#pragma unroll
    for (int e = 0; e < 8; e++) smem.dbp[sm][sv + e] = dbs[e];
    __syncthreads();
    if (tid < 64 && j0 + tid < a.PC) {
      float s = smem.dbp[0][tid];
      for (int i = 1; i < 32; i++) s += smem.dbp[i][tid];
      a.db[j0 + tid] = a.accum ? a.db[j0 + tid] + s : s;
    }
    __syncthreads();
  }

#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++)
#pragma unroll
      for (int q = 0; q < 4; q++)
        smem.out[wr * 32 + mi * 16 + fk * 4 + q][wc * 32 + ni * 16 + fr] =
            acc[mi][ni][q];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int idx = tid + i * 256;
    const int row = idx >> 4, c4 = (idx & 15) * 4;
    const int j = j0 + row, t = t0 + c4;
    if (j < a.PC && t < a.QC) {  // QC % 4 == 0: the four columns are inside
      float* o = a.dw + (long)j * a.QC + t;
      float4 v = {smem.out[row][c4], smem.out[row][c4 + 1],
                  smem.out[row][c4 + 2], smem.out[row][c4 + 3]};
      if (a.dwvec) {
        if (a.accum) {
          const float4 p = *(const float4*)o;
          v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        *(float4*)o = v;
      } else {
        o[0] = a.accum ? o[0] + v.x : v.x;
        o[1] = a.accum ? o[1] + v.y : v.y;
        o[2] = a.accum ? o[2] + v.z : v.z;
        o[3] = a.accum ? o[3] + v.w : v.w;
      }
    }
  }
}

template <bool A>
__global__ __launch_bounds__(256) void k_se_excite_bwd(SeBwdArgs a) {
  __shared__ SeBwdSmem smem;
  const int bid = blockIdx.x;
  if (bid < a.nrow) {
    se_rowmat_tile<A>(a, (bid / a.ntq) * 64, (bid % a.ntq) * 64, smem);
  } else {
    const int id = bid - a.nrow;
    se_outer_tile<A>(a, (id / a.ntq) * 64, (id % a.ntq) * 64, smem);
  }
}

// -------------------------------------------------------------- launchers --
static long g_se_fwd = 0, g_se_bwd = 0;

static bool se_aligned16(const void* p) { return ((size_t)p & 15) == 0; }

extern "C" {

// H·W splits of the squeeze and of the backward reduce: enough workgroups to
// cover the chip's 256 CUs twice, at least 256 pixels per split, and 1 below
// 512 pixels.  HZ_SE_SPLITS overrides the rule; it is read at every call so
// one process can run several values.  The result leaves no split empty.
int se_splits(int N, int HW) {
  long want = env_long("HZ_SE_SPLITS", 0);
  if (want <= 0)
    want = HW < 512 ? 1 : std::min((512 + N - 1) / N, HW / 256);
  want = std::max(1L, std::min(want, (long)std::min(HW, 64)));
  const int chunk = (int)((HW + want - 1) / want);
  return (HW + chunk - 1) / chunk;
}

void se_launch_counts(long* fwd, long* bwd) {
  *fwd = g_se_fwd;
  *bwd = g_se_bwd;
}

void launch_se_fwd(const void* u, const void* res, void* y, const void* w1,
                   const float* b1, const void* w2, const float* b2,
                   float* part, float* s, float* h, float* g, int N, int HW,
                   int C, int Cr, int splits, int act, hipStream_t st) {
  const int chunk = (HW + splits - 1) / splits;
  const int L = C / 8;
  k_se_pool<0><<<dim3(N, splits), 256, 0, st>>>(
      (const bf16*)u, nullptr, nullptr, part, HW, C, chunk);
  k_se_excite<<<dim3((C + 63) / 64, (N + 15) / 16), 256, 0, st>>>(
      part, (const bf16*)w1, b1, (const bf16*)w2, b2, s, h, g, N, C, Cr,
      splits, 1.f / (float)HW);
  const int pb = (256 / L) * SE_PIX_ITERS;
  const dim3 grid((HW + pb - 1) / pb, N);
  const bf16 *up = (const bf16*)u, *rp = (const bf16*)res;
  bf16* yp = (bf16*)y;
  if (res && act)
    k_se_scale<true, true><<<grid, 256, 0, st>>>(up, g, rp, yp, HW, C);
  else if (res)
    k_se_scale<true, false><<<grid, 256, 0, st>>>(up, g, rp, yp, HW, C);
  else if (act)
    k_se_scale<false, true><<<grid, 256, 0, st>>>(up, g, rp, yp, HW, C);
  else
    k_se_scale<false, false><<<grid, 256, 0, st>>>(up, g, rp, yp, HW, C);
  g_se_fwd += 3;
}

void launch_se_bwd(const void* dy, const void* y, const void* u,
                   const void* w1, const void* w2, const float* s,
                   const float* h, const float* g, float* part, float* dh,
                   float* ds, void* du, void* dres, float* dw1, float* db1,
                   float* dw2, float* db2, int N, int HW, int C, int Cr,
                   int splits, int act, int accum, hipStream_t st) {
  const int chunk = (HW + splits - 1) / splits;
  const int L = C / 8;
  const bf16 *dyp = (const bf16*)dy, *yp = (const bf16*)y,
             *up = (const bf16*)u;
  if (act)
    k_se_pool<2><<<dim3(N, splits), 256, 0, st>>>(up, dyp, yp, part, HW, C,
                                                  chunk);
  else
    k_se_pool<1><<<dim3(N, splits), 256, 0, st>>>(up, dyp, nullptr, part, HW,
                                                  C, chunk);
  const int nm = (N + 63) / 64, ntc = (C + 63) / 64, ntr = (Cr + 63) / 64;
  SeBwdArgs a{};
  a.N = N;
  a.splits = splits;
  a.accum = accum;
  // stage A: P columns = C, Q / W columns = Cr
  a.part = part;
  a.gate = g;
  a.q = h;
  a.w = (const bf16*)w2;
  a.mask = h;
  a.out = dh;
  a.dw = dw2;
  a.db = db2;
  a.PC = C;
  a.QC = Cr;
  a.dwvec = se_aligned16(dw2) ? 1 : 0;
  a.nrow = nm * ntr;
  a.ntq = ntr;
  k_se_excite_bwd<true><<<a.nrow + ntc * ntr, 256, 0, st>>>(a);
  // stage B: P columns = Cr, Q / W columns = C
  a.part = nullptr;
  a.gate = nullptr;
  a.p = dh;
  a.q = s;
  a.w = (const bf16*)w1;
  a.mask = nullptr;
  a.out = ds;
  a.dw = dw1;
  a.db = db1;
  a.PC = Cr;
  a.QC = C;
  a.dwvec = se_aligned16(dw1) ? 1 : 0;
  a.nrow = nm * ntc;
  a.ntq = ntc;
  k_se_excite_bwd<false><<<a.nrow + ntr * ntc, 256, 0, st>>>(a);
  const int pb = (256 / L) * SE_PIX_ITERS;
  const dim3 grid((HW + pb - 1) / pb, N);
  bf16 *dup = (bf16*)du, *drp = (bf16*)dres;
  const float inv = 1.f / (float)HW;
  if (dres && act)
    k_se_bwd_apply<true, true><<<grid, 256, 0, st>>>(dyp, yp, g, ds, dup, drp,
                                                     HW, C, inv);
  else if (dres)
    k_se_bwd_apply<true, false><<<grid, 256, 0, st>>>(dyp, yp, g, ds, dup, drp,
                                                      HW, C, inv);
  else if (act)
    k_se_bwd_apply<false, true><<<grid, 256, 0, st>>>(dyp, yp, g, ds, dup, drp,
                                                      HW, C, inv);
  else
    k_se_bwd_apply<false, false><<<grid, 256, 0, st>>>(dyp, yp, g, ds, dup,
                                                       drp, HW, C, inv);
  g_se_bwd += 4;
}

}  // extern "C"
