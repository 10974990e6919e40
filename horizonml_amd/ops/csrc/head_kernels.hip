// Wide classifier head for gfx950 (MI355X, CDNA4): the linear layer at
// Out > 16 on the bf16 16×16×32 MFMA, and the cross-entropy loss at NC > 32
// with one wave per row.  Reached through launch_linear_* / launch_ce_* in
// elem_kernels.hip, which own the dispatch; Out ≤ 16 and NC ≤ 32 never come
// here.  docs/KERNELS.md, "Wide head".
//
// MFMA fragment maps (v_mfma_f32_16x16x32_bf16), lane = (r = lane & 15,
// g = lane >> 4):
//   A  lane holds A[row r][k = 8g .. 8g+7]
//   B  lane holds B[k = 8g .. 8g+7][col r]
//   D  lane holds D[row 4g + q][col r], q = 0..3
// No kernel here uses atomics except the CE loss scalar, so the linear
// results agree bitwise between two runs and serve deterministic mode too.
#include "common.h"

// ---------------------------------------------------------------- forward --
// logits[B,Out] f32 = x[B,In] bf16 · W[Out,In]ᵀ bf16 + b.
//
// Both operands are K-major, so a fragment IS a 16-byte global load: lane
// (r, g) reads row r at k0 + 8g.  Nothing goes through LDS on the way in.
//   block   one strip of 16 classes × up to 64 batch rows;
//           grid = (ceil(Out/16), ceil(B/64))
//   waves   split K inside the block.  The unit is a PAIR of adjacent 32-k
//           MFMA steps (64 k = the whole 128-byte line a lane touched);
//           wave w takes pairs w, w+4, ...  W is streamed once per row tile.
//           A wave keeps ceil(rows/16) accumulators.
//   tails   rows ≥ B, classes ≥ Out and k ≥ In are zeros selected into the
//           fragment — EXEC stays all ones at every MFMA.  In % 8 == 0 makes
//           a lane's 8 k all inside or all outside.
//   end     the four partial tiles meet in LDS (16 KB) and are summed in
//           wave order 0..3, then the bias is added.
// Rounding chain of one output: ≤ ceil(In/64)/4·2 MFMA steps in a wave (16
// at In = 2048), 32 products inside a step, 3 combines, 1 bias add.
struct HeadFrag {
  V8 w[2];
  V8 x[4][2];
};

__global__ __launch_bounds__(256) void k_head_fwd(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ y, int B, int In,
    int Out) {
  // [wave][mi][q][g][r]: a wave's store of one (mi, q) is 64 floats in a row
  __shared__ float part[4][1024];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int j0 = blockIdx.x * 16, m0 = blockIdx.y * 64;
  const int nfrag = min(4, (B - m0 + 15) >> 4);  // block-uniform
  const int npair = (In + 63) >> 6;
  const bool wok = j0 + r < Out;
  const bf16* wrow = w + (long)(j0 + r) * In;

  auto load = [&](int kp, HeadFrag& f) {
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int k = kp * 64 + h * 32 + g * 8;
      const bool kok = k < In;
      if (wok && kok) f.w[h].u = *(const uint4*)(wrow + k);
      else f.w[h].u = uint4{0, 0, 0, 0};
#pragma unroll
      for (int mi = 0; mi < 4; mi++) {
        const int row = m0 + mi * 16 + r;
        if (mi < nfrag && row < B && kok)
          f.x[mi][h].u = *(const uint4*)(x + (long)row * In + k);
        else
          f.x[mi][h].u = uint4{0, 0, 0, 0};
      }
    }
  };

  f32x4 acc[4] = {};
  HeadFrag cur, nx;
  if (wave < npair) load(wave, cur);
  for (int kp = wave; kp < npair; kp += 4) {
    // the next pair's loads are in flight while this pair computes
    const bool more = kp + 4 < npair;
    if (more) load(kp + 4, nx);
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int mi = 0; mi < 4; mi++)
        if (mi < nfrag)
          acc[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              cur.x[mi][h].v, cur.w[h].v, acc[mi], 0, 0, 0);
    if (more) cur = nx;
  }

#pragma unroll
  for (int mi = 0; mi < 4; mi++)
#pragma unroll
    for (int q = 0; q < 4; q++)
      part[wave][(mi * 4 + q) * 64 + lane] = acc[mi][q];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int e = tid + i * 256;
    const int row = m0 + (e >> 8) * 16 + ((e >> 4) & 3) * 4 + ((e >> 6) & 3);
    const int j = j0 + (e & 15);
    if (row < B && j < Out) {
      float v = part[0][e];
      v += part[1][e];
      v += part[2][e];
      v += part[3][e];
      y[(long)row * Out + j] = v + (b ? b[j] : 0.f);
    }
  }
}

// --------------------------------------------------------------- backward --
// dx[B,In] bf16 = dy · W;  dW[Out,In] f32 (+)= dyᵀ · x;  db[Out] f32 (+)= Σ_b dy
// in ONE launch.  A block's role comes from blockIdx.x and is block-uniform;
// the dx blocks come first, they have the long K loop (Out / 32 steps).
//
// f32 dy on the bf16 matrix unit.  dy is the f32 dlogits of the loss kernel
// and the former kernels used it at f32; one rounding to bf16 would cost 2⁻⁹
// per term.  Each value is split into three bf16 terms
//   hi = bf16(dy), mid = bf16(dy − hi), lo = bf16(dy − hi − mid).
// Each remainder is exact in f32 and lo needs at most 8 bits, so
// hi + mid + lo == dy for normal f32.  Every fragment pair gets three MFMAs,
// smallest term first; a bf16×bf16 product is exact in the f32 accumulator,
// so only the accumulation order differs from an f32 dot product.  The build
// is -ffast-math: a denormal remainder may flush to zero (an error below
// 2⁻¹²⁶ per term).  The head is far from MFMA-bound, so tripling the MFMA
// count is the cheap way to leave training numerics where they were.
//
// EXEC rule (docs/KERNELS.md): the transposed reads and the MFMAs run with
// EXEC all ones.  Role, tile and loop bounds are block-uniform, no role
// returns early, and rows ≥ B, classes ≥ Out and columns ≥ In are ZEROS in
// the images and fragments, never masked lanes.
DEV void split3(const float (&d)[8], V8& hi, V8& mid, V8& lo) {
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

// dy[b][j .. j+7] (j % 8 == 0), zeros past B / Out.  vec4: rows are 16-byte
// aligned (Out % 4 == 0 and an aligned base; block-uniform).
DEV void load_dy8(const float* __restrict__ dy, int B, int Out, int b, int j,
                  bool vec4, float (&d)[8]) {
  const float* p = dy + (long)b * Out + j;
  if (b < B && vec4 && j + 8 <= Out) {
    const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
    d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
    d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++)
      d[e] = (b < B && j + e < Out) ? p[e] : 0.f;
  }
}

DEV bf16x8 read_tr_frag(const bf16* img, int off) {
  const bf16x4 lo = lds_read_tr16(img + off);
  const bf16x4 hi = lds_read_tr16(img + off + 4 * 64);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

union HeadBwdSmem {
  struct {  // dW role: [32 b][64] images of lds_tr_off<64>, 16 KB
    __attribute__((aligned(16))) bf16 X[32 * 64];
    __attribute__((aligned(16))) bf16 D[3][32 * 64];  // lo, mid, hi
  } w;
  __attribute__((aligned(16))) bf16 W[32 * 64];  // dx role: [32 j][64 t]
  float out[64][65];  // dW epilogue: [class][column]
  float dbp[32][64];  // db partials: [tile row][class]
};

// dx role: 64 batch rows × 64 input columns, reduction over Out in steps of
// 32.  W[j][t] is reduction-rows × output-columns — dgrad's KRSC B tile — so
// it is staged as it lies and read transposed.  dy[b][j] is contiguous along
// the reduction: each lane loads its 8 f32, splits them in registers, and
// those are the A fragments.
DEV void head_dx_tile(const float* __restrict__ dy,
                      const bf16* __restrict__ w, bf16* __restrict__ dx,
                      int B, int In, int Out, int m0, int t0, bool vec4,
                      HeadBwdSmem& smem) {
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // W tile: j row, 8-wide t
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
  auto load_tile = [&](int j0) {
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
      load_dy8(dy, B, Out, m0 + wr * 32 + mi * 16 + fr, j0 + fk * 8, vec4,
               a_nx[mi]);
    if (j0 + sm < Out && t0 + sv < In)
      w_nx.u = *(const uint4*)(w + (long)(j0 + sm) * In + t0 + sv);
    else
      w_nx.u = uint4{0, 0, 0, 0};
  };

  f32x4 acc[2][2] = {};
  load_tile(0);
  for (int j0 = 0; j0 < Out; j0 += 32) {
    *(V8*)&smem.W[lds_tr_off<64>(sm, sv)] = w_nx;
    V8 af[3][2];  // lo, mid, hi
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
      split3(a_nx[mi], af[2][mi], af[1][mi], af[0][mi]);
    __syncthreads();
    if (j0 + 32 < Out) load_tile(j0 + 32);
    bf16x8 bf[2];
#pragma unroll
    for (int ni = 0; ni < 2; ni++) bf[ni] = read_tr_frag(smem.W, boff[ni]);
#pragma unroll
    for (int s = 0; s < 3; s++)
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int ni = 0; ni < 2; ni++)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[s][mi].v, bf[ni], acc[mi][ni], 0, 0, 0);
    __syncthreads();
  }
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      const int t = t0 + wc * 32 + ni * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int bi = m0 + wr * 32 + mi * 16 + fk * 4 + q;
        if (bi < B && t < In) dx[(long)bi * In + t] = f2b(acc[mi][ni][q]);
      }
    }
}

// dW role: 64 classes × 64 input columns, reduction over B in steps of 32.
// dy[b][j] and x[b][t] are both reduction-rows × output-columns, the shape
// of wgrad's tiles: one 16-byte LDS store per vec8 into lds_tr_off<64>
// images (x, and the three dy terms), fragments by two transposed reads.
// The accumulators go back through LDS to coalesced float4 rows of dW.
// Blocks of input tile 0 also sum their 64 dy columns over B — the unsplit
// f32 values, per tile row first, then the 32 tile rows in order.
DEV void head_dw_tile(const float* __restrict__ dy,
                      const bf16* __restrict__ x, float* __restrict__ dw,
                      float* __restrict__ db, int B, int In, int Out, int j0,
                      int t0, bool vec4, bool dwvec, int accum,
                      HeadBwdSmem& smem) {
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // tile row b, 8-wide j / t
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
  float d_nx[8], dbs[8];
  V8 x_nx;
  auto load_tile = [&](int b0) {
    load_dy8(dy, B, Out, b0 + sm, j0 + sv, vec4, d_nx);
    if (b0 + sm < B && t0 + sv < In)
      x_nx.u = *(const uint4*)(x + (long)(b0 + sm) * In + t0 + sv);
    else
      x_nx.u = uint4{0, 0, 0, 0};
  };
#pragma unroll
  for (int e = 0; e < 8; e++) dbs[e] = 0.f;

  f32x4 acc[2][2] = {};
  const int soff = lds_tr_off<64>(sm, sv);
  load_tile(0);
  for (int b0 = 0; b0 < B; b0 += 32) {
    V8 hi, mid, lo;
    split3(d_nx, hi, mid, lo);
    *(V8*)&smem.w.X[soff] = x_nx;
    *(V8*)&smem.w.D[0][soff] = lo;
    *(V8*)&smem.w.D[1][soff] = mid;
    *(V8*)&smem.w.D[2][soff] = hi;
#pragma unroll
    for (int e = 0; e < 8; e++) dbs[e] += d_nx[e];
    __syncthreads();
    if (b0 + 32 < B) load_tile(b0 + 32);
    bf16x8 bf[2];
#pragma unroll
    for (int ni = 0; ni < 2; ni++) bf[ni] = read_tr_frag(smem.w.X, boff[ni]);
#pragma unroll
    for (int s = 0; s < 3; s++) {
      bf16x8 af[2];
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
        af[mi] = read_tr_frag(smem.w.D[s], aoff[mi]);
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int ni = 0; ni < 2; ni++)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    }
    __syncthreads();
  }

  if (db != nullptr && t0 == 0) {  // block-uniform
#pragma unroll
    for (int e = 0; e < 8; e++) smem.dbp[sm][sv + e] = dbs[e];
    __syncthreads();
    if (tid < 64 && j0 + tid < Out) {
      float s = smem.dbp[0][tid];
      for (int i = 1; i < 32; i++) s += smem.dbp[i][tid];
      db[j0 + tid] = accum ? db[j0 + tid] + s : s;
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
    if (j < Out && t < In) {  // In % 8 == 0: the four columns are all inside
      float* o = dw + (long)j * In + t;
      float4 v = {smem.out[row][c4], smem.out[row][c4 + 1],
                  smem.out[row][c4 + 2], smem.out[row][c4 + 3]};
      if (dwvec) {
        if (accum) {
          const float4 p = *(const float4*)o;
          v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        *(float4*)o = v;
      } else {
        o[0] = accum ? o[0] + v.x : v.x;
        o[1] = accum ? o[1] + v.y : v.y;
        o[2] = accum ? o[2] + v.z : v.z;
        o[3] = accum ? o[3] + v.w : v.w;
      }
    }
  }
}

// ndx = dx blocks (0 when dx is not wanted), ntx = ceil(In / 64).
__global__ __launch_bounds__(256) void k_head_bwd(
    const float* __restrict__ dy, const bf16* __restrict__ x,
    const bf16* __restrict__ w, bf16* __restrict__ dx,
    float* __restrict__ dw, float* __restrict__ db, int B, int In, int Out,
    int accum, int ndx, int ntx, int vec4, int dwvec) {
  __shared__ HeadBwdSmem smem;
  const int bid = blockIdx.x;
  if (bid < ndx) {
    head_dx_tile(dy, w, dx, B, In, Out, (bid / ntx) * 64, (bid % ntx) * 64,
                 vec4 != 0, smem);
  } else {
    const int id = bid - ndx;
    head_dw_tile(dy, x, dw, db, B, In, Out, (id / ntx) * 64, (id % ntx) * 64,
                 vec4 != 0, dwvec != 0, accum, smem);
  }
}

// ---------------------------------------------------------- cross-entropy --
// Wide CE (NC > 32): one wave per batch row, four rows per block; lanes
// stride the classes, so every global access is coalesced.  The row is read
// once and kept in LDS (4 rows × NC f32, dynamic): each lane re-reads only
// the elements it wrote, so no barrier is needed, and no register array is
// indexed at run time.  Max and Σexp close with xor-shuffle trees.  The row
// maths is ce_row<LS>'s (elem_kernels.hip): lse in f32, __expf / __logf,
// the one-hot and the label-smoothing gradient.  Lane 0 adds the row's share
// of the loss into loss[0], which the caller zeroed.
template <bool LS>
DEV void ce_wide_body(const float* __restrict__ logits,
                      const long* __restrict__ target,
                      float* __restrict__ loss, float* __restrict__ dlogits,
                      int B, int NC, float eps) {
  extern __shared__ float ce_rows[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;  // a whole wave; the kernel has no barrier
  float* sr = ce_rows + wave * NC;
  const float* row = logits + (long)b * NC;
  float* drow = dlogits + (long)b * NC;
  float mx = row[0], sx = 0.f;
  for (int j = lane; j < NC; j += 64) {
    const float v = row[j];
    sr[j] = v;
    mx = fmaxf(mx, v);
    if (LS) sx += v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  float se = 0.f;
  for (int j = lane; j < NC; j += 64) se += __expf(sr[j] - mx);
  se = wave_reduce_sum(se);
  const float lse = __logf(se) + mx;
  const int t = (int)target[b];
  float li = lse - row[t];
  const float invB = 1.f / (float)B;
  if (LS) {
    sx = wave_reduce_sum(sx);
    li = (1.f - eps) * li + eps * (lse - sx / (float)NC);
    const float on = 1.f - eps, off = eps / (float)NC;
    for (int j = lane; j < NC; j += 64) {
      const float p = __expf(sr[j] - lse);
      drow[j] = (p - (j == t ? on : 0.f) - off) * invB;
    }
  } else {
    for (int j = lane; j < NC; j += 64) {
      const float p = __expf(sr[j] - lse);
      drow[j] = (p - (j == t ? 1.f : 0.f)) * invB;
    }
  }
  if (lane == 0) atomicAdd(loss, li / (float)B);
}

__global__ __launch_bounds__(256) void k_ce_wide(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC) {
  ce_wide_body<false>(logits, target, loss, dlogits, B, NC, 0.f);
}

__global__ __launch_bounds__(256) void k_ce_ls_wide(
    const float* __restrict__ logits, const long* __restrict__ target,
    float* __restrict__ loss, float* __restrict__ dlogits, int B, int NC,
    float eps) {
  ce_wide_body<true>(logits, target, loss, dlogits, B, NC, eps);
}

// -------------------------------------------------------------- launchers --
static bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

extern "C" {

void launch_head_fwd(const void* x, const void* w, const float* b, float* y,
                     int B, int In, int Out, hipStream_t st) {
  dim3 grid((Out + 15) / 16, (B + 63) / 64);
  k_head_fwd<<<grid, 256, 0, st>>>((const bf16*)x, (const bf16*)w, b, y, B,
                                   In, Out);
}

void launch_head_bwd(const float* dy, const void* x, const void* w, void* dx,
                     float* dw, float* db, int B, int In, int Out, int accum,
                     hipStream_t st) {
  const int ntx = (In + 63) / 64;
  const int ndx = dx ? ((B + 63) / 64) * ntx : 0;
  const int ndw = ((Out + 63) / 64) * ntx;
  const int vec4 = (Out % 4 == 0) && aligned16(dy);
  k_head_bwd<<<ndx + ndw, 256, 0, st>>>(
      dy, (const bf16*)x, (const bf16*)w, (bf16*)dx, dw, db, B, In, Out,
      accum, ndx, ntx, vec4, aligned16(dw) ? 1 : 0);
}

void launch_ce_wide(const float* logits, const long* target, float* loss,
                    float* dlogits, int B, int NC, float eps, int ls,
                    hipStream_t st) {
  const size_t lds = sizeof(float) * 4 * (size_t)NC;  // NC ≤ CE_WIDE_MAX_NC
  if (ls)
    k_ce_ls_wide<<<(B + 3) / 4, 256, lds, st>>>(logits, target, loss,
                                                dlogits, B, NC, eps);
  else
    k_ce_wide<<<(B + 3) / 4, 256, lds, st>>>(logits, target, loss, dlogits,
                                             B, NC);
}

}  // extern "C"
