// Implicit-GEMM convolution kernels for gfx950 (MI355X, CDNA4).
//
// One MFMA tile template serves three modes:
//   MODE 0  GEMM      C[M,N]  = A[M,Kd] · B[N,Kd]^T            (bf16 in, bf16 out)
//   MODE 1  CONV_FWD  y[m,ko] = Σ_{r,s,c} x[patch] · W[ko,r,s,c]   (NHWC / KRSC)
//   MODE 2  CONV_DGRAD dx[m,c] = Σ_{r,s,ko} dz[mapped] · Wr[r,s,c,ko] (RSCK)
//   MODE 2 + KRSC     the same dgrad with B read from the KRSC weight
//                     W[ko,r,s,c] itself (transposed LDS read, see below)
//
// Geometry: 64×64 block tile, BK=32 K-steps, 256 threads = 4 waves in 2×2,
// each wave computes a 32×32 sub-tile as 2×2 mfma_f32_16x16x32_bf16
// fragments.  A/B tiles are LDS-staged with +8-element row padding.
//
// Latency design (these conv shapes are tiny — batch 64 CIFAR gives
// M=64..16k, so kernels are latency-bound, not throughput-bound):
//  * double-buffered LDS with ONE barrier per K-step and 2-deep register
//    prefetch: tile k+2's loads are in flight while tile k computes, so
//    the ~900-cycle HBM latency hides even at 1 block/CU;
//  * split-K: when a long K loop would serialize on an underfilled grid
//    (thresholds measured per direction — see pick_splitk /
//    conv_dgrad_splitk), the K reduction is partitioned over blockIdx.z
//    into per-split f32 slabs summed by the consumer pass (stats_reduce /
//    bn_apply forward, cast[+fused BN reduce] backward) — no atomics.
//
// The non-split forward epilogue also accumulates per-channel BN batch
// statistics (Σy, Σy²) via wave shuffle reduction + one atomicAdd per
// 16-lane group, so a training conv+BN block is 2 kernels total
// (north-star fused conv+BN+ReLU).
#include "common.h"  // ConvP, MagicP and make_magic come from launch.h

// ---------------------------------------------------------------- staging --
// Tap window (launch.h, clip_taps): R, S, Kd are the window's and the k index
// runs over the window.  CLIP is a template flag of every gather and of the
// kernels built on them: CLIP = false is the whole-filter address arithmetic
// (no origin, Rf = R, Sf = S) and compiles to what it compiled to before the
// window existed; CLIP = true adds the origin (r0, s0) to the patch
// coordinates and addresses weights / dW through the full Rf×Sf filter.  The
// host picks the flag per conv (taps_clipped), and instantiates CLIP = true
// for the 64-wide latency tiles only: a clipped conv has a 1-2 pixel map.
template <int MODE, bool CLIP = false>
DEV int a_addr(const ConvP& p, const MagicP& mg, int m, int k, bool& valid) {
  if (MODE == 0) {
    valid = (m < p.M) & (k < p.Kd);
    return m * p.Kd + k;
  } else if (MODE == 1) {
    // x gather: m -> (n,ho,wo), k -> (r,s,c); index decompositions via
    // magic-number division (the emulated u32 divides dominated the VALU)
    unsigned n = fdiv(m, mg, 0), hw = fmod(m, n, mg, 0);
    unsigned ho = fdiv(hw, mg, 1), wo = fmod(hw, ho, mg, 1);
    unsigned r = fdiv(k, mg, 2), rm = fmod(k, r, mg, 2);
    unsigned sx = fdiv(rm, mg, 3), c = fmod(rm, sx, mg, 3);
    const int ph = CLIP ? p.pad - p.r0 : p.pad;
    const int pw = CLIP ? p.pad - p.s0 : p.pad;
    int hi = (int)ho * p.str - ph + (int)r;
    int wi = (int)wo * p.str - pw + (int)sx;
    valid = (m < p.M) & (k < p.Kd) & (hi >= 0) & (hi < p.H) & (wi >= 0) & (wi < p.W);
    return (((int)n * p.H + hi) * p.W + wi) * p.C + (int)c;
  } else {
    // dz gather (dgrad): m -> (n,hi,wi) over input dims, k -> (r,s,ko)
    unsigned n = fdiv(m, mg, 0), hw = fmod(m, n, mg, 0);
    unsigned hi = fdiv(hw, mg, 1), wi = fmod(hw, hi, mg, 1);
    unsigned r = fdiv(k, mg, 2), rm = fmod(k, r, mg, 2);
    unsigned sx = fdiv(rm, mg, 3), ko = fmod(rm, sx, mg, 3);
    const int ph = CLIP ? p.pad - p.r0 : p.pad;
    const int pw = CLIP ? p.pad - p.s0 : p.pad;
    int hs = (int)hi + ph - (int)r, ws = (int)wi + pw - (int)sx;
    bool ok = (m < p.M) & (k < p.Kd) & (hs >= 0) & (ws >= 0) &&
              (hs % p.str == 0) && (ws % p.str == 0);
    int ho = hs / p.str, wo = ws / p.str;  // str is 1 or 2: cheap
    ok = ok && (ho < p.Ho) && (wo < p.Wo);
    valid = ok;
    return (((int)n * p.Ho + ho) * p.Wo + wo) * p.K + (int)ko;
  }
}

// window tap index rs = r*S + s at reduction index k (slot 2 = S * channels)
// -> tap (r0 + r)*Sf + s0 + s of the filter as stored
DEV int full_tap(const ConvP& p, const MagicP& mg, int k, int rs) {
  int r = (int)fdiv(k, mg, 2);
  return (p.r0 + r) * p.Sf + p.s0 + (rs - r * p.S);
}

template <int MODE, bool CLIP = false>
DEV int b_addr(const ConvP& p, const MagicP& mg, int n, int k, int Ntot,
               bool& valid) {
  if (MODE == 2) {
    // W_rsck[(r*S+s)*C + c][ko] with k = (r*S+s)*K + ko, n = c
    unsigned rs = fdiv(k, mg, 3), ko = fmod(k, rs, mg, 3);
    valid = (n < Ntot) & (k < p.Kd);
    if (CLIP) rs = (unsigned)full_tap(p, mg, k, (int)rs);
    return ((int)rs * p.C + n) * p.K + (int)ko;
  }
  valid = (n < Ntot) & (k < p.Kd);
  if (MODE == 1 && CLIP) {
    // W[n][r0+r][s0+s][c]: window row r sits (Sf - S)*C further on per row
    unsigned r = fdiv(k, mg, 2);
    return n * (p.Rf * p.Sf * p.C) +
           (p.r0 * p.Sf + p.s0 + (int)r * (p.Sf - p.S)) * p.C + k;
  }
  return n * p.Kd + k;
}

template <int MODE, bool VEC, bool CLIP = false>
DEV V8 load8_a(const bf16* __restrict__ src, const ConvP& p,
               const MagicP& mg, int m, int k) {
  V8 v;
  if (VEC) {
    bool ok;
    int a = a_addr<MODE, CLIP>(p, mg, m, k, ok);
    if (ok) v.u = *(const uint4*)(src + a);
    else v.u = uint4{0, 0, 0, 0};
  } else if (MODE == 1) {
    // scalar x-gather (C not a multiple of 8, e.g. the stem's C=3): one
    // (r,s,c) decomposition per vec8 and incremental carry across the 8
    // elements — the naive per-element a_addr costs ~5 integer divides
    // each and dominated the stem conv
    int n = m / (p.Ho * p.Wo), hw = m % (p.Ho * p.Wo);
    int ho = hw / p.Wo, wo = hw % p.Wo;
    int r = k / (p.S * p.C), rm = k % (p.S * p.C);
    int s = rm / p.C, c = rm % p.C;
    int hi = ho * p.str - (CLIP ? p.pad - p.r0 : p.pad) + r;
    int wi = wo * p.str - (CLIP ? p.pad - p.s0 : p.pad) + s;
    const bool mok = m < p.M;
    int kk = k;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      bool ok = mok && kk < p.Kd && hi >= 0 && hi < p.H && wi >= 0 &&
                wi < p.W;
      v.e[e] = ok ? src[((n * p.H + hi) * p.W + wi) * p.C + c] : (bf16)0.f;
      kk++;
      if (++c == p.C) {
        c = 0;
        ++wi;
        if (++s == p.S) {
          s = 0;
          wi -= p.S;
          ++r;
          ++hi;
        }
      }
    }
  } else {
    for (int e = 0; e < 8; e++) {
      bool ok;
      int a = a_addr<MODE, CLIP>(p, mg, m, k + e, ok);
      v.e[e] = ok ? src[a] : (bf16)0.f;
    }
  }
  return v;
}

template <int MODE, bool VEC, bool CLIP = false>
DEV V8 load8_b(const bf16* __restrict__ src, const ConvP& p,
               const MagicP& mg, int n, int k, int Ntot) {
  V8 v;
  if (VEC) {
    bool ok;
    int a = b_addr<MODE, CLIP>(p, mg, n, k, Ntot, ok);
    if (ok) v.u = *(const uint4*)(src + a);
    else v.u = uint4{0, 0, 0, 0};
  } else {
    for (int e = 0; e < 8; e++) {
      bool ok;
      int a = b_addr<MODE, CLIP>(p, mg, n, k + e, Ntot, ok);
      v.e[e] = ok ? src[a] : (bf16)0.f;
    }
  }
  return v;
}

// ------------------------------------------- KRSC-direct dgrad B operand --
// dgrad's B operand is B[k][n] with k = (r*S+s)*K + ko, n = c.  In the KRSC
// weight a k row is contiguous along c, so a K-step tile (32 k rows × TN
// columns) is staged AS IT LIES IN MEMORY into a [32][TN] LDS image and the
// MFMA B-fragment (8 consecutive k of one column per lane) is fetched with
// the gfx950 transposed read ds_read_b64_tr_b16 — no RSCK copy of the
// weights is needed.  Operand values and K order equal MODE 2 on the RSCK
// image, so the result is bitwise the same.
//
// Image: row pitch TN*2 bytes, the row's 32-byte chunks (16 columns) XORed
// with a function of the row.  One transposed read serves, per 32-lane
// half, two 4-row blocks 8 rows apart in the same 16 columns (groups g and
// g+1: rows 8g+q and 8g+8+q).  A pitch that is a multiple of 32 B leaves
// rows r and r+8 on the same banks, and a 16-B-odd pitch (the +8 pad of the
// row-major image) always overlaps two of the eight rows, so the rows are
// separated by the swizzle instead: with 128-B rows (TN=64) the row parity
// picks the half of the 256-B bank row and bits {1,3} of the row pick the
// chunk; with 256-B rows (TN=128) bits {0,1,3} do.  The eight rows of a
// half then cover all 64 banks once: conflict-free by the bank rule.  The
// swizzle moves whole 32-byte chunks, so the 16-byte staging stores and
// the 8-byte-aligned transposed reads both stay inside one chunk, and the
// second read of a fragment (rows +4) is the first one's address + 4 rows.
// The wgrad operand tiles ([32 m][k3], [32 m][ko]) use the same image.
template <int TN>
DEV int lds_tr_off(int k, int n) {
  const int f = TN == 64 ? (((k >> 1) & 1) | (((k >> 3) & 1) << 1))
                         : ((k & 3) | (((k >> 3) & 1) << 2));
  return k * TN + ((((n >> 4) ^ f)) << 4) + (n & 15);
}

// One vec8 along c of k row `k`: W[ko][r][s][n .. n+7], (rs, ko) from one
// fdiv/fmod.  Rows past kend and columns past C are zero-filled.
template <bool VEC, bool CLIP = false>
DEV V8 load8_b_krsc(const bf16* __restrict__ src, const ConvP& p,
                    const MagicP& mg, int n, int k, int kend, int Ntot) {
  V8 v;
  unsigned rs = fdiv(k, mg, 3), ko = fmod(k, rs, mg, 3);
  const bool kok = k < kend;
  const int a =
      CLIP ? ((int)ko * p.Rf * p.Sf + full_tap(p, mg, k, (int)rs)) * p.C + n
           : ((int)ko * p.R * p.S + (int)rs) * p.C + n;
  if (VEC) {
    if (kok && n < Ntot) v.u = *(const uint4*)(src + a);
    else v.u = uint4{0, 0, 0, 0};
  } else {
    for (int e = 0; e < 8; e++)
      v.e[e] = (kok && n + e < Ntot) ? src[a + e] : (bf16)0.f;
  }
  return v;
}

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// ds_read_b64_tr_b16.  Needs EXEC all ones: call it from block-uniform
// control flow only, with every lane's address inside the image.
DEV bf16x4 lds_read_tr16(const bf16* sp) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)sp);
}

// ------------------------------------------------------------- main tile --
#define LDA 40  // 32 + 8 pad; row stride 80 B

// SPLIT: each blockIdx.z writes its f32 partial into its own slab
// ws_out[z][M][Ntot] (no atomics, no pre-zeroing — the consumer pass sums
// the slabs); otherwise write bf16 into Y (+ optional stats).
//
// TM×TN block tile (waves in a fixed 2×2 grid, wave tile (TM/2)×(TN/2)):
//  * 64×64 (default) — the LATENCY tile for the CIFAR-shape grids: small
//    LDS footprint, shortest prologue, best when the grid underfills the
//    256 CUs and every block must hide HBM latency alone;
//  * 128×64 / 128×128 — THROUGHPUT tiles for ImageNet-shaped work
//    (selected by pick_tile when the tiled grid still fills the chip):
//    each wave runs 8/16 MFMAs per K-step against the same 6/8 LDS
//    fragment reads, lifting the MFMA:issue ratio that caps the 64×64
//    tile at ~2% of the bf16 peak on ResNet50@224 (r50_224_pmc_mfma.txt).
//
// KRSC (MODE 2 only): B is the KRSC weight; Bs holds the swizzled [32][TN]
// image of lds_tr_off() in place of the [TN][LDA] one and the B fragments come
// from transposed reads.  The A side, the accumulators, the K order and the
// epilogue are shared with the RSCK form.
template <int MODE, bool VECA, bool VECB, bool STATS, bool SPLIT,
          int TM = 64, int TN = 64, bool KRSC = false, bool CLIP = false>
__global__ __launch_bounds__(256) void k_conv_mfma(
    const bf16* __restrict__ A, const bf16* __restrict__ Bw,
    bf16* __restrict__ Y, float* __restrict__ ws_out,
    float* __restrict__ stats, ConvP p, MagicP mg, int Ntot, int kchunk,
    int accum) {
  // Double-buffered LDS, ONE barrier per K-step, 2-deep register
  // prefetch: tile k+2's global loads are in flight while tile k computes,
  // so the ~900-cycle HBM latency hides even at 1 block/CU.
  constexpr int AC = TM / 64;   // A stage chunks per thread (vec8 each)
  constexpr int BC = TN / 64;
  constexpr int MI = TM / 32;   // 16-row m fragments per wave
  constexpr int NI = TN / 32;
  constexpr int WM = TM / 2, WN = TN / 2;
  static_assert(!KRSC || MODE == 2, "KRSC is a dgrad B layout");
  static_assert(!KRSC || TN == 64 || TN == 128,
                "lds_tr_off covers TN 64/128");
  __shared__ __attribute__((aligned(16))) bf16 As[2][TM * LDA];
  __shared__ __attribute__((aligned(16))) bf16 Bs[2][TN * LDA];  // ≥ 32*TN

  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
  const int kbeg = SPLIT ? blockIdx.z * kchunk : 0;
  const int kend = SPLIT ? min(p.Kd, kbeg + kchunk) : p.Kd;
  const int tid = threadIdx.x;
  const int srow = tid >> 2, scol = (tid & 3) * 8;  // 1 vec8 per thread
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
  // KRSC staging: chunk j of a thread is vec8 (tid + 256 j) of the 32 × TN
  // tile, TN/8 per k row — a wave loads whole contiguous rows of c
  const int bkrow = tid / (TN / 8), bncol = (tid % (TN / 8)) * 8;
  constexpr int BKSTEP = 256 / (TN / 8);  // k rows between a thread's chunks

  // B tile k-origin `kt`, chunk j -> registers; registers -> LDS buffer b
  auto load_b = [&](int j, int kt) -> V8 {
    if (KRSC)
      return load8_b_krsc<VECB, CLIP>(Bw, p, mg, n0 + bncol,
                                      kt + j * BKSTEP + bkrow, kend, Ntot);
    return load8_b<MODE, VECB, CLIP>(Bw, p, mg, n0 + j * 64 + srow,
                                     kt + scol, Ntot);
  };
  auto store_b = [&](int b, int j, const V8& v) {
    if (KRSC)
      *(V8*)&Bs[b][lds_tr_off<TN>(j * BKSTEP + bkrow, bncol)] = v;
    else
      *(V8*)&Bs[b][(j * 64 + srow) * LDA + scol] = v;
  };
  // KRSC fragment addresses (T10 map): lane 4q+pp of 16-lane group fk
  // supplies row 8 fk + q, columns 4 pp .. 4 pp + 3 of the fragment's 16
  int boff[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ni++)
    boff[ni] = lds_tr_off<TN>(fk * 8 + (fr >> 2),
                            wc * WN + ni * 16 + (fr & 3) * 4);

  f32x4 acc[MI][NI] = {};

  // prologue: tile 0 -> LDS[0]; tile 1 -> registers
#pragma unroll
  for (int j = 0; j < AC; j++) {
    V8 a0 = load8_a<MODE, VECA, CLIP>(A, p, mg, m0 + j * 64 + srow,
                                      kbeg + scol);
    *(V8*)&As[0][(j * 64 + srow) * LDA + scol] = a0;
  }
#pragma unroll
  for (int j = 0; j < BC; j++) store_b(0, j, load_b(j, kbeg));
  V8 a_nx[AC], b_nx[BC];
  if (kbeg + 32 < kend) {
#pragma unroll
    for (int j = 0; j < AC; j++)
      a_nx[j] = load8_a<MODE, VECA, CLIP>(A, p, mg, m0 + j * 64 + srow,
                                          kbeg + 32 + scol);
#pragma unroll
    for (int j = 0; j < BC; j++) b_nx[j] = load_b(j, kbeg + 32);
  }
  __syncthreads();

  int buf = 0;
  for (int k0 = kbeg; k0 < kend; k0 += 32) {
    // stage tile k+1 from registers into the OTHER buffer (its readers
    // synchronized at the previous barrier), then issue tile k+2's loads
    if (k0 + 32 < kend) {
#pragma unroll
      for (int j = 0; j < AC; j++)
        *(V8*)&As[buf ^ 1][(j * 64 + srow) * LDA + scol] = a_nx[j];
#pragma unroll
      for (int j = 0; j < BC; j++) store_b(buf ^ 1, j, b_nx[j]);
      if (k0 + 64 < kend) {
#pragma unroll
        for (int j = 0; j < AC; j++)
          a_nx[j] = load8_a<MODE, VECA, CLIP>(A, p, mg, m0 + j * 64 + srow,
                                              k0 + 64 + scol);
#pragma unroll
        for (int j = 0; j < BC; j++) b_nx[j] = load_b(j, k0 + 64);
      }
    }
    bf16x8 af[MI], bf[NI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
      af[mi] =
          *(const bf16x8*)&As[buf][(wr * WM + mi * 16 + fr) * LDA + fk * 8];
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      if (KRSC) {
        // block-uniform: every lane of every wave issues both reads
        bf16x4 lo = lds_read_tr16(&Bs[buf][boff[ni]]);
        bf16x4 hi = lds_read_tr16(&Bs[buf][boff[ni] + 4 * TN]);
        bf[ni] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      } else {
        bf[ni] =
            *(const bf16x8*)&Bs[buf][(wc * WN + ni * 16 + fr) * LDA + fk * 8];
      }
    }
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    buf ^= 1;
    __syncthreads();
  }

  // Epilogue. D fragment: col = lane&15 (=fr), row = fk*4 + q.
  float ssum[NI], ssq[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ni++) ssum[ni] = ssq[ni] = 0.f;
#pragma unroll
  for (int mi = 0; mi < MI; mi++) {
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      int gn = n0 + wc * WN + ni * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int gm = m0 + wr * WM + mi * 16 + fk * 4 + q;
        if (gm < p.M && gn < Ntot) {
          float v = acc[mi][ni][q];
          if (SPLIT) {
            ws_out[(long)blockIdx.z * p.M * Ntot + (long)gm * Ntot + gn] = v;
          } else {
            long yi = (long)gm * Ntot + gn;
            if (accum) v += b2f(Y[yi]);  // fused residual-junction add
            Y[yi] = f2b(v);
            if (STATS) {
              ssum[ni] += v;
              ssq[ni] += v * v;
            }
          }
        }
      }
    }
  }
  if (STATS && !SPLIT && stats != nullptr) {
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      float s = ssum[ni] + __shfl_xor(ssum[ni], 16, 64);
      s += __shfl_xor(s, 32, 64);
      float s2 = ssq[ni] + __shfl_xor(ssq[ni], 16, 64);
      s2 += __shfl_xor(s2, 32, 64);
      int gn = n0 + wc * WN + ni * 16 + fr;
      if (fk == 0 && gn < Ntot) {
        atomicAdd(&stats[gn], s);
        atomicAdd(&stats[Ntot + gn], s2);
      }
    }
  }
}

// ------------------------------------------------------------------ wgrad --
// dW[ko][k3] += Σ_m patch(m,k3) · dz(m,ko);  dW is KRSC flat [Ntot][Kd] f32.
// MFMA formulation: the reduction axis is m.  In the transposed-scatter
// form (TR = false) both operands are staged TRANSPOSED into LDS ([k3][m]
// and [ko][m]) during the gather (coalesced global vec8 reads, 8 strided b16
// LDS writes per thread), which makes the MFMA fragment reads contiguous
// ds_read_b128; the row-major form (below) is the default.  Output tile
// 64(k3)×64(ko), m reduced 32-deep per MFMA step, msplit-way M parallelism.
//
// Epilogue is ATOMIC-FREE (measured: the former per-element f32 atomicAdd
// into dW cost ~12.5 µs per million atomics and dominated wgrad — see
// profiles/bench_r01_opt1_graph_stats.txt): the accumulator tile is
// transposed through LDS into [ko][k3] row order and written with plain
// coalesced float4 accesses — read-modify-write into the pre-zeroed
// gradient when msplit == 1 (single writer per element; += preserves
// multi-backward accumulation), else pure stores into a per-split slab
// ws[z][Ntot][Kd] that the reduce kernel sums into the gradient.
//
// Deferred/batched mode (the flat fast path): all convs' wgrads of one
// backward run as ONE kernel — every task's (tile, z) blocks are in flight
// together, so the chip fills without oversplitting M, and 2 launches
// replace ~40 (bind.cpp::flush_wgrad).
//
// Row-major form (TR, the default): the operand tiles are [32 m][k3] and
// [32 m][ko] as they come out of the gather — exactly the shape of dgrad's
// KRSC B tile (reduction rows × output columns).  Each thread's vec8 goes
// into the swizzled image of lds_tr_off() with ONE 16-byte store instead of
// eight swizzled ds_write_b16, and the MFMA fragments (8 consecutive m of one
// k3 / ko column per lane) are fetched with two ds_read_b64_tr_b16 each, as
// MODE 2 + KRSC forms bf[ni].  Lane (fr, fk) ends up with rows 8fk..8fk+7 of
// column fr — what the ds_read_b128 of the transposed image delivers — so
// operand values, the m order inside an MFMA and the MFMA order are those of
// the transposed form and dW is bitwise the same.
//   EXEC rule: the transposed reads run with EXEC all ones.  mbeg/mend, the
// task lookup and the vec flag are block-uniform and there is no early
// return; rows ≥ M, k3 ≥ Kd and ko ≥ K are ZEROS in the image (the loaders
// zero-fill), never masked lanes.
//   The m-loop keeps one LDS buffer, two barriers per K-step and a one-deep
// register prefetch: k_conv_mfma's double-buffered loop was built on top of
// this body and measured no faster for any flagship task (docs/STATUS.md,
// "Measured negative results").
// TR == false is the transposed-scatter body, kept for A/B timing and as
// the bitwise reference of the tests (HZ_WGRAD_TR=0 / set_wgrad_tr(false)).
#define LDW 40  // 32 m + 8 pad

// TK3: k3-tile width (64 default; 128 for big-Kd large-M convs — halves
// the Dz re-read traffic and doubles MFMA per staging write).  The out
// image keeps an odd f32 row stride (65 / 131) for conflict-free stores.
template <int TK3, int TKO = 64>
union WgradSmemT {
  struct {
    bf16 At[TK3 * LDW];  // [k3][m]
    bf16 Dt[TKO * LDW];  // [ko][m]
  } s;
  struct {  // TR: [32 m][TK3 | TKO], swizzled by lds_tr_off
    __attribute__((aligned(16))) bf16 A[32 * TK3];
    __attribute__((aligned(16))) bf16 D[32 * TKO];
  } r;
  float out[64][TK3 == 64 ? 65 : 131];  // transposed epilogue staging
};
using WgradSmem = WgradSmemT<64, 64>;

// m-loop of the row-major form: accumulates rows [mbeg, mend) into acc.
template <bool VECA, int TK3, int TKO, bool CLIP>
DEV void wgrad_mloop_tr(const bf16* __restrict__ X,
                        const bf16* __restrict__ Dz, const ConvP& p,
                        const MagicP& mg, int Ntot, int k3_0, int n0,
                        int mbeg, int mend, WgradSmemT<TK3, TKO>& smem,
                        f32x4 (&acc)[TK3 / 32][TKO / 32]) {
  constexpr int AC = TK3 / 64, DC = TKO / 64;
  constexpr int MI = TK3 / 32, NI = TKO / 32;
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // m row, 8-wide k3/ko chunk
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;

  V8 a_nx[AC], d_nx[DC];
  // tile with m-origin mt -> registers (zero-filled past M / Kd / K)
  auto load_tile = [&](int mt) {
#pragma unroll
    for (int j = 0; j < AC; j++)
      a_nx[j] =
          load8_a<1, VECA, CLIP>(X, p, mg, mt + sm, k3_0 + j * 64 + sv);
#pragma unroll
    for (int j = 0; j < DC; j++) {
      int m = mt + sm, n = n0 + j * 64 + sv;
      if (m < p.M && n < Ntot)
        d_nx[j].u = *(const uint4*)(Dz + (long)m * Ntot + n);
      else
        d_nx[j].u = uint4{0, 0, 0, 0};
    }
  };
  bf16* At = smem.r.A;  // [32 m][TK3]
  bf16* Dt = smem.r.D;  // [32 m][TKO]
  // fragment addresses (T10 map): lane 4q+pp of 16-lane group fk supplies
  // row 8 fk + q, columns 4 pp .. 4 pp + 3 of the fragment's 16
  int aoff[MI], doff[NI];
#pragma unroll
  for (int mi = 0; mi < MI; mi++)
    aoff[mi] = lds_tr_off<TK3>(fk * 8 + (fr >> 2),
                               wr * (TK3 / 2) + mi * 16 + (fr & 3) * 4);
#pragma unroll
  for (int ni = 0; ni < NI; ni++)
    doff[ni] = lds_tr_off<TKO>(fk * 8 + (fr >> 2),
                               wc * (TKO / 2) + ni * 16 + (fr & 3) * 4);

  load_tile(mbeg);
  for (int m0 = mbeg; m0 < mend; m0 += 32) {
    // registers -> LDS as the tile lies in memory: one 16-byte store a chunk
#pragma unroll
    for (int j = 0; j < AC; j++)
      *(V8*)&At[lds_tr_off<TK3>(sm, j * 64 + sv)] = a_nx[j];
#pragma unroll
    for (int j = 0; j < DC; j++)
      *(V8*)&Dt[lds_tr_off<TKO>(sm, j * 64 + sv)] = d_nx[j];
    __syncthreads();
    if (m0 + 32 < mend) load_tile(m0 + 32);
    // block-uniform: every lane of every wave issues all the reads
    bf16x8 af[MI], bf[NI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
      bf16x4 lo = lds_read_tr16(&At[aoff[mi]]);
      bf16x4 hi = lds_read_tr16(&At[aoff[mi] + 4 * TK3]);
      af[mi] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      bf16x4 lo = lds_read_tr16(&Dt[doff[ni]]);
      bf16x4 hi = lds_read_tr16(&Dt[doff[ni] + 4 * TKO]);
      bf[ni] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    __syncthreads();
  }
}

template <bool VECA, int TK3 = 64, int TKO = 64, bool TR = false,
          bool CLIP = false>
DEV void wgrad_tile(const bf16* __restrict__ X, const bf16* __restrict__ Dz,
                    float* __restrict__ out, const ConvP& p,
                    const MagicP& mg, int Ntot, int mchunk, int tx, int ty,
                    int z, bool split, WgradSmemT<TK3, TKO>& smem) {
  constexpr int AC = TK3 / 64;   // A staging chunks per thread
  constexpr int DC = TKO / 64;   // Dz staging chunks per thread
  constexpr int MI = TK3 / 32;   // k3 fragments per wave
  constexpr int NI = TKO / 32;   // ko fragments per wave
  bf16* At = smem.s.At;   // [k3][m]
  bf16* Dt = smem.s.Dt;   // [ko][m]
  const int k3_0 = tx * TK3, n0 = ty * TKO;
  const int mbeg = z * mchunk;
  const int mend = min(p.M, mbeg + mchunk);
  const int tid = threadIdx.x;
  const int sm = tid >> 3, sv = (tid & 7) * 8;  // m-lane, 8-wide k3/ko chunk
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;

  f32x4 acc[MI][NI] = {};

  if (TR) {
    wgrad_mloop_tr<VECA, TK3, TKO, CLIP>(X, Dz, p, mg, Ntot, k3_0, n0, mbeg,
                                         mend, smem, acc);
  } else {
  // transposed-scatter m-loop, unchanged
  V8 a_nx[AC], d_nx[DC];
#pragma unroll
  for (int j = 0; j < AC; j++)
    a_nx[j] =
        load8_a<1, VECA, CLIP>(X, p, mg, mbeg + sm, k3_0 + j * 64 + sv);
#pragma unroll
  for (int j = 0; j < DC; j++) {
    int m = mbeg + sm, n = n0 + j * 64 + sv;
    if (m < p.M && n < Ntot)
      d_nx[j].u = *(const uint4*)(Dz + (long)m * Ntot + n);
    else
      d_nx[j].u = uint4{0, 0, 0, 0};
  }
  const int smlo = sm & 7, smhi = sm >> 3;
  for (int m0 = mbeg; m0 < mend; m0 += 32) {
    // transposed scatter into LDS: element (m=sm, k3=sv+e) -> At[sv+e][sm']
    // with the m 8-chunk XOR-swizzled by row&3 (8-way -> 2-way write banks)
#pragma unroll
    for (int j = 0; j < AC; j++)
#pragma unroll
      for (int e = 0; e < 8; e++) {
        int row = j * 64 + sv + e;
        int smx = smlo | (((smhi ^ row) & 3) << 3);
        At[row * LDW + smx] = a_nx[j].e[e];
      }
#pragma unroll
    for (int j = 0; j < DC; j++)
#pragma unroll
      for (int e = 0; e < 8; e++) {
        int row = j * 64 + sv + e;
        int smx = smlo | (((smhi ^ row) & 3) << 3);
        Dt[row * LDW + smx] = d_nx[j].e[e];
      }
    __syncthreads();
    if (m0 + 32 < mend) {
#pragma unroll
      for (int j = 0; j < AC; j++)
        a_nx[j] = load8_a<1, VECA, CLIP>(X, p, mg, m0 + 32 + sm,
                                         k3_0 + j * 64 + sv);
#pragma unroll
      for (int j = 0; j < DC; j++) {
        int m = m0 + 32 + sm, n = n0 + j * 64 + sv;
        if (m < p.M && n < Ntot)
          d_nx[j].u = *(const uint4*)(Dz + (long)m * Ntot + n);
        else
          d_nx[j].u = uint4{0, 0, 0, 0};
      }
    }
    bf16x8 af[MI], bf[NI];
#pragma unroll
    for (int mi = 0; mi < MI; mi++) {
      int row = wr * (TK3 / 2) + mi * 16 + fr;
      af[mi] = *(const bf16x8*)&At[row * LDW + ((fk ^ row) & 3) * 8];
    }
#pragma unroll
    for (int ni = 0; ni < NI; ni++) {
      int row = wc * (TKO / 2) + ni * 16 + fr;
      bf[ni] = *(const bf16x8*)&Dt[row * LDW + ((fk ^ row) & 3) * 8];
    }
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
      for (int ni = 0; ni < NI; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
    __syncthreads();
  }
  }  // !TR
  // D: col (=ko) = fr, row (=k3) = fk*4+q.  Transpose through the 64-ko
  // LDS image, one pass per 64-ko slab (TKO=128: pass p uses only the
  // wc==p waves' accumulators; every thread joins the global store).
  float* dst = out + (split ? (long)z * Ntot * (long)p.Kd : 0L);
  constexpr int CCH = TK3 / 4;  // k3 span per thread in the store pass
  const int ko_r = tid >> 2, cch = (tid & 3) * CCH;
#pragma unroll
  for (int pass = 0; pass < TKO / 64; pass++) {
    __syncthreads();  // LDS union / previous pass done
    if (TKO == 64 || wc == pass) {
#pragma unroll
      for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int ni = 0; ni < NI; ni++) {
          int ko_l = wc * (TKO / 2) + ni * 16 + fr - pass * 64;
#pragma unroll
          for (int q = 0; q < 4; q++)
            smem.out[ko_l][wr * (TK3 / 2) + mi * 16 + fk * 4 + q] =
                acc[mi][ni][q];
        }
    }
    __syncthreads();
    const int gko = n0 + pass * 64 + ko_r;
    if (CLIP && !split) {
      // clipped task writing dW itself: row gko at the full-filter pitch,
      // the k3 run mapped to its taps; dead taps are neither read nor
      // written.  With C % 4 == 0 a float4 never straddles a tap.
      if (gko < Ntot) {
        const long row = (long)gko * (p.Rf * p.Sf * p.C) +
                         (p.r0 * p.Sf + p.s0) * p.C;
        const int skip = (p.Sf - p.S) * p.C;
        if ((p.C & 3) == 0 && k3_0 + cch + CCH <= p.Kd) {
#pragma unroll
          for (int e = 0; e < CCH; e += 4) {
            const int k3 = k3_0 + cch + e;
            float* d4 = &dst[row + k3 + (int)fdiv(k3, mg, 2) * skip];
            float4 v = *(const float4*)&smem.out[ko_r][cch + e];
            float4 d = *(const float4*)d4;
            v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
            *(float4*)d4 = v;
          }
        } else {
          for (int e = 0; e < CCH && k3_0 + cch + e < p.Kd; e++) {
            const int k3 = k3_0 + cch + e;
            dst[row + k3 + (int)fdiv(k3, mg, 2) * skip] +=
                smem.out[ko_r][cch + e];
          }
        }
      }
    } else if (gko < Ntot) {
      long base = (long)gko * p.Kd + k3_0 + cch;
      if (k3_0 + cch + CCH <= p.Kd) {
#pragma unroll
        for (int e = 0; e < CCH; e += 4) {
          float4 v = *(const float4*)&smem.out[ko_r][cch + e];
          if (!split) {  // accumulate into .grad (single writer; RMW safe)
            float4 d = *(const float4*)&dst[base + e];
            v.x += d.x; v.y += d.y; v.z += d.z; v.w += d.w;
          }
          *(float4*)&dst[base + e] = v;
        }
      } else {
        for (int e = 0; e < CCH && k3_0 + cch + e < p.Kd; e++)
          dst[base + e] =
              smem.out[ko_r][cch + e] + (split ? 0.f : dst[base + e]);
      }
    }
  }
}

template <bool VECA, bool TR, bool CLIP>
__global__ __launch_bounds__(256) void k_wgrad(
    const bf16* __restrict__ X, const bf16* __restrict__ Dz,
    float* __restrict__ dW, ConvP p, MagicP mg, int Ntot, int mchunk) {
  __shared__ WgradSmem smem;
  wgrad_tile<VECA, 64, 64, TR, CLIP>(X, Dz, dW, p, mg, Ntot, mchunk,
                                     blockIdx.x, blockIdx.y, blockIdx.z,
                                     gridDim.z > 1, smem);
}

// Slab reduce of a clipped task (WredTask::Kd > 0, launch.h): the slabs are
// dense over the tap window, dW is the full filter.  Sums slab elements
// [begin, end) and adds them into their taps; thread `tid` of `nthr`.
DEV long wred_dst(const WredTask& t, unsigned i) {
  unsigned ko = i / (unsigned)t.Kd, k3 = i - ko * (unsigned)t.Kd;
  return (long)ko * t.KdF + t.org + k3 + (k3 / (unsigned)t.SC) * t.skip;
}

DEV void wred_scatter(const WredTask& t, long begin, long end, long tid,
                      long nthr) {
  // every term a multiple of 4 (C % 4 == 0): a float4 stays inside one tap
  if (((t.Kd | t.SC | t.KdF | t.org | t.skip) & 3) == 0) {
    for (long i4 = begin + tid * 4; i4 < end; i4 += nthr * 4) {
      float4 v = *(const float4*)&t.ws[i4];
      for (int z = 1; z < t.msplit; z++) {
        float4 w = *(const float4*)&t.ws[(long)z * t.n + i4];
        v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
      }
      float4* dp = (float4*)&t.dW[wred_dst(t, (unsigned)i4)];
      float4 d = *dp;
      d.x += v.x; d.y += v.y; d.z += v.z; d.w += v.w;
      *dp = d;
    }
  } else {
    for (long i = begin + tid; i < end; i += nthr) {
      float v = t.ws[i];
      for (int z = 1; z < t.msplit; z++) v += t.ws[(long)z * t.n + i];
      t.dW[wred_dst(t, (unsigned)i)] += v;
    }
  }
}

// Σ over msplit wgrad slabs [z][n] -> dW[n] (+=; dW pre-zeroed or fresh).
__global__ __launch_bounds__(256) void k_wgrad_reduce(WredTask t) {
  if (t.Kd > 0) {  // block-uniform
    wred_scatter(t, 0, t.n, (long)blockIdx.x * blockDim.x + threadIdx.x,
                 (long)gridDim.x * blockDim.x);
    return;
  }
  const float* __restrict__ ws = t.ws;
  float* __restrict__ dW = t.dW;
  const long n = t.n;
  const int msplit = t.msplit;
  long i4 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (; i4 + 4 <= n; i4 += stride) {
    float4 v = *(const float4*)&ws[i4];
    for (int z = 1; z < msplit; z++) {
      float4 w = *(const float4*)&ws[(long)z * n + i4];
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    float4 d = *(float4*)&dW[i4];
    d.x += v.x; d.y += v.y; d.z += v.z; d.w += v.w;
    *(float4*)&dW[i4] = d;
  }
  // tail (Kd*K not divisible by 4)
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    long tail = n & ~3L;
    for (long i = tail + threadIdx.x; i < n; i += 4) {
      float v = ws[i];
      for (int z = 1; z < msplit; z++) v += ws[(long)z * n + i];
      dW[i] += v;
    }
  }
}

// ------------------------------------------------- batched (deferred) wgrad --
// One launch computes every pending conv's weight gradient: all tasks'
// (tile, z) blocks are in flight together so msplit can stay small
// (mchunk ≈ 512 rows) and the grid still fills 256 CUs without atomics.
// Task tables travel as kernel arguments by value — no staging buffers,
// hipGraph-capture-safe.  WgradBatchArgs / WredBatchArgs: launch.h.
template <int TK3, int TKO, bool TR>
__global__ __launch_bounds__(256) void k_wgrad_batched(WgradBatchArgs a) {
  int bid = blockIdx.x;
  int i = 0;
  while (i + 1 < a.n && bid >= a.t[i + 1].base) i++;
  const WgradTask& t = a.t[i];
  int local = bid - t.base;
  int nt = t.tx * t.ty;
  int z = local / nt, rem = local - z * nt;
  int ty = rem / t.tx, tx = rem - ty * t.tx;
  __shared__ WgradSmemT<TK3, TKO> smem;
  const bf16* X = (const bf16*)t.X;
  const bf16* Dz = (const bf16*)t.Dz;
  // clipped tasks ride in the TK3 = 64 classes (bind.cpp, tk3_of); the task
  // and so each of these tests is block-uniform
  constexpr bool CL = TK3 == 64;
  if (CL && ((t.p.R != t.p.Rf) | (t.p.S != t.p.Sf))) {
    if (t.vec)
      wgrad_tile<true, TK3, TKO, TR, CL>(X, Dz, t.out, t.p, t.mg, t.Ntot,
                                         t.mchunk, tx, ty, z, t.msplit > 1,
                                         smem);
    else
      wgrad_tile<false, TK3, TKO, TR, CL>(X, Dz, t.out, t.p, t.mg, t.Ntot,
                                          t.mchunk, tx, ty, z, t.msplit > 1,
                                          smem);
  } else if (t.vec)
    wgrad_tile<true, TK3, TKO, TR>(X, Dz, t.out, t.p, t.mg, t.Ntot, t.mchunk,
                                   tx, ty, z, t.msplit > 1, smem);
  else
    wgrad_tile<false, TK3, TKO, TR>(X, Dz, t.out, t.p, t.mg, t.Ntot, t.mchunk,
                                    tx, ty, z, t.msplit > 1, smem);
}

__global__ __launch_bounds__(256) void k_wgrad_reduce_batched(
    WredBatchArgs a) {
  int bid = blockIdx.x;
  int i = 0;
  while (i + 1 < a.n && bid >= a.t[i + 1].base) i++;
  const WredTask& t = a.t[i];
  if (t.Kd > 0) {  // block-uniform
    const long begin = (long)(bid - t.base) * 1024;
    wred_scatter(t, begin, min(t.n, begin + 1024), threadIdx.x, 256);
    return;
  }
  long i4 = ((long)(bid - t.base) * 256 + threadIdx.x) * 4;
  if (i4 + 4 <= t.n) {
    float4 v = *(const float4*)&t.ws[i4];
    for (int z = 1; z < t.msplit; z++) {
      float4 w = *(const float4*)&t.ws[(long)z * t.n + i4];
      v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
    }
    float4 d = *(float4*)&t.dW[i4];
    d.x += v.x; d.y += v.y; d.z += v.z; d.w += v.w;
    *(float4*)&t.dW[i4] = d;
  } else {
    for (long j = i4; j < t.n; j++) {
      float v = t.ws[j];
      for (int z = 1; z < t.msplit; z++) v += t.ws[(long)z * t.n + j];
      t.dW[j] += v;
    }
  }
}

// ------------------------------------------------------------- launchers --
static inline int cdiv_h(int a, int b) { return (a + b - 1) / b; }

// Split-K heuristic.  Split-K costs a whole consumer chain (f32 slabs +
// stats_reduce/cast + slab re-reads), so it only pays when a non-split
// launch would serialize a long K loop on an underfilled grid: measured on
// MI355X, non-split wins for Kd ≤ ~1152 even at 32–64 workgroups (the
// K-loop is ~18–36 latency-hidden iterations), while layer3/4 shapes
// (Kd ≥ 2304, ≤16 tiles) still want the split.
static inline int pick_splitk(int tiles, int Kd) {
  // tunables (read once): grid-fill target and minimum Kd that justifies
  // the split-K consumer chain
  // r02 re-sweep: 256 splits the layer3/4-class long-K forwards too:
  // r50@224 10.01 -> 9.05 ms same-box, CIFAR bs=1024 +3%, bs=64 flat
  static const int tile_min = (int)env_long("HZ_SK_TILES", 256);
  static const int kd_min = (int)env_long("HZ_SK_KD", 1024);
  if (tiles >= tile_min || Kd < kd_min) return 1;
  int sk = cdiv_h(256, tiles);
  int maxsk = cdiv_h(Kd, 32);
  if (sk > maxsk) sk = maxsk;
  if (sk > 32) sk = 32;
  return sk;
}

static inline int pick_tile(int M, int N);
static inline int pick_tile_dgrad(int M, int N);
// Tile class of one conv.  A clipped conv (tap window, a 1-2 pixel map)
// takes the 64x64 latency tile: the CLIP kernels exist for that tile only.
static inline int conv_tile(const ConvP& p) {
  return taps_clipped(p) ? 0 : pick_tile(p.M, p.K);
}
// p: forward geometry
static inline int conv_tile_dgrad(const ConvP& p) {
  return taps_clipped(p) ? 0 : pick_tile_dgrad(p.Nb * p.H * p.W, p.C);
}

// Fill-split (HZ_SK_FILL / HZ_SK_FILL_DG, default 0 = off): when the
// throughput 128x128 tile is picked but its grid lands under `fillmin`
// blocks (r50@224 bs=32 mid-layers: 98-196 blocks on 256 CUs), split K
// across blockIdx.z to recover occupancy instead of falling back to the
// latency tile.  The split path pays the f32 workspace + consumer pass,
// so this only makes sense for long-K shapes (kd floor re-used).
static int sk_fill(int dgrad) {
  static const int vf = (int)env_long("HZ_SK_FILL", 0);
  // swept on r50@224 bs=32 (same box): 8.536 -> 8.485 ms; the fwd
  // variant (HZ_SK_FILL) measured flat and stays off — its split
  // drags the stats pass + slab re-reads
  static const int vd = (int)env_long("HZ_SK_FILL_DG", 256);
  return dgrad ? vd : vf;
}

static int fill_splitk(int blocks128, int Kd, int fillmin) {
  int sk = cdiv_h(fillmin, blocks128);
  int maxsk = cdiv_h(Kd, 32);
  if (sk > maxsk) sk = maxsk;
  if (sk > 8) sk = 8;
  return sk;
}

extern "C" int conv_fwd_splitk(ConvP p) {
  int tiles = cdiv_h(p.K, 64) * cdiv_h(p.M, 64);
  // HZ_SK_CLIP_FULL=0: feed a clipped conv's window Kd to the picker below
  // like any other conv (A/B knob; sweep in profiles/r10_fwd_split_policy.txt)
  static const int clip_full = (int)env_long("HZ_SK_CLIP_FULL", 1);
  if (clip_full && taps_clipped(p)) {
    // A clipped conv keeps the dispatch class of its whole filter (split-K
    // slabs + the owner BN at small M, which tests/test_bn_owner_gpu.py pins
    // for the layer4 shapes): the decision is taken on the full Kd, and the
    // window only shortens the K loop.  It never splits finer than the whole
    // filter did — more slabs for less K would only add consumer traffic —
    // nor finer than the window has K-steps.
    const int kd_full = p.Rf * p.Sf * p.C;
    int sk = pick_splitk(tiles, kd_full);
    if (sk > 1) {
      sk = cdiv_h(kd_full, cdiv_h(cdiv_h(kd_full, sk), 32) * 32);
      sk = min(sk, cdiv_h(p.Kd, 32));
    }
    return sk;
  }
  int sk = pick_splitk(tiles, p.Kd);
  if (sk == 1 && sk_fill(0) > 0 && p.Kd >= 512 && conv_tile(p) == 2) {
    int blocks = cdiv_h(p.M, 128) * cdiv_h(p.K, 128);
    if (blocks < sk_fill(0)) return fill_splitk(blocks, p.Kd, sk_fill(0));
  }
  return sk;
}

extern "C" int conv_dgrad_splitk(ConvP p) {
  // dgrad geometry: M=Nb*H*W rows, Kd=R*S*K, N=C.  dgrad has its own Kd
  // threshold: its split path costs only the cast pass (often fused with
  // the upstream conv's BN reduce), so splitting pays at smaller Kd than
  // the forward's split (which drags a stats pass + slab re-reads).
  static const int kd_min_dg = (int)env_long("HZ_SK_KD_DG", 512);
  // swept: r50@224 9.05 -> 8.89 ms; CIFAR flat
  static const int tile_min_dg = (int)env_long("HZ_SK_TILES_DG", 256);
  int tiles = cdiv_h(p.C, 64) * cdiv_h(p.Nb * p.H * p.W, 64);
  int Kd = p.R * p.S * p.K;
  if (tiles >= tile_min_dg || Kd < kd_min_dg) {
    int M = p.Nb * p.H * p.W;
    if (sk_fill(1) > 0 && Kd >= 512 && conv_tile_dgrad(p) == 2) {
      int blocks = cdiv_h(M, 128) * cdiv_h(p.C, 128);
      if (blocks < sk_fill(1)) return fill_splitk(blocks, Kd, sk_fill(1));
    }
    return 1;
  }
  int sk = cdiv_h(256, tiles);
  int maxsk = cdiv_h(Kd, 32);
  if (sk > maxsk) sk = maxsk;
  if (sk > 32) sk = 32;
  return sk;
}

// ------------------------------------------------------ stem direct conv --
// Specialized forward for the ImageNet stem (C=3, 7x7, stride 2, pad 3,
// K<=64): the generic implicit-GEMM path must SCALAR-gather x (C=3 defeats
// vec8) and runs short K loops per 64x64 tile — measured 209 us at
// ResNet50@224 bs=32 / ~24 us at the CIFAR parity point.  Here the whole
// weight tensor (<=64x147 bf16) lives in LDS zero-PADDED to 32 k-slots per
// filter row (one K-step == one filter row r), and the needed x rows are
// staged once per block with a 9-element halo — the im2col "gather"
// becomes one linear LDS read, because for fixed r the (s,c) flattening is
// stride-1 in NHWC memory: patch element j = s*3+c sits at
// x[row][(wo*2-3)*3 + j].  Pad-k products are exact zeros (weight slots
// zeroed; the A slack reads stay inside the staged buffer, so finite).
//
// Block: rows_pb output rows x wo_pad columns (<=128 outputs) of ONE
// image, all K channels.  Waves 2x2: wave tile 64(m) x 32(K): 8 MFMA per
// K-step, 7 K-steps.  A-fragment LDS reads are 4x b32 (patch base is only
// 4-byte aligned: wo*6 bf16); W rows use a 232-element pitch (16B-aligned
// rows, 116-dword stride => conflict-free 16-lane b128 reads).
#define STEM_WPITCH 232
template <bool STATS>
__global__ __launch_bounds__(256) void k_stem_conv(
    const bf16* __restrict__ X, const bf16* __restrict__ Wk,
    bf16* __restrict__ Y, float* __restrict__ stats, ConvP p, int rows_pb,
    int wo_pad, int xpitch, int bpi) {
  extern __shared__ bf16 sm[];
  bf16* Wl = sm;                       // [64][STEM_WPITCH]
  bf16* Xl = sm + 64 * STEM_WPITCH;    // [rows_pb*2+5][xpitch]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;

  // --- stage weights: W flat [K][147] -> Wl[K][r*32 + j] (j<21), 0 pad --
  for (int i = tid; i < 64 * STEM_WPITCH; i += 256) {
    int ch = i / STEM_WPITCH, col = i - ch * STEM_WPITCH;
    int r = col >> 5, j = col & 31;
    bf16 v = (bf16)0.f;
    if (ch < p.K && r < 7 && j < 21 && col < 7 * 32)
      v = Wk[ch * 147 + r * 21 + j];
    Wl[i] = v;
  }

  // --- stage x rows with 9-element left halo, zero outside [0,W) -------
  const int n = blockIdx.x / bpi;
  const int ho0 = (blockIdx.x - n * bpi) * rows_pb;
  const int nrows = rows_pb * 2 + 5;   // input rows hi0 .. hi0+nrows-1
  const int hi0 = ho0 * 2 - 3;
  const int rowlen = p.W * 3;
  for (int i = tid; i < nrows * xpitch; i += 256) {
    int rr = i / xpitch, col = i - rr * xpitch;
    int hi = hi0 + rr;
    bf16 v = (bf16)0.f;
    int e = col - 9;  // halo: col 9 == x element 0 of the row
    if (hi >= 0 && hi < p.H && e >= 0 && e < rowlen)
      v = X[((long)(n * p.H + hi) * p.W) * 3 + e];
    Xl[i] = v;
  }
  __syncthreads();

  // --- MFMA main loop: 7 K-steps (one filter row each) ------------------
  f32x4 acc[4][2] = {};
  int abase[4];  // lane's A base (clamped memory-safe for invalid m)
#pragma unroll
  for (int mi = 0; mi < 4; mi++) {
    int ml = wr * 64 + mi * 16 + fr;
    int hl = ml / wo_pad;
    int wo = ml - hl * wo_pad;
    if (hl >= rows_pb) hl = rows_pb - 1;   // slack lanes: clamp (discarded)
    abase[mi] = hl * 2 * xpitch + wo * 6 + fk * 8;
  }
#pragma unroll
  for (int r = 0; r < 7; r++) {
    bf16x8 af[4], bf[2];
#pragma unroll
    for (int mi = 0; mi < 4; mi++) {
      // 4-byte-aligned LDS read path (base is even-element)
      const uint32_t* xu = (const uint32_t*)&Xl[abase[mi] + r * xpitch];
      union { uint32_t u[4]; bf16x8 v; } a;
      a.u[0] = xu[0];
      a.u[1] = xu[1];
      a.u[2] = xu[2];
      a.u[3] = xu[3];
      af[mi] = a.v;
    }
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      int ch = wc * 32 + ni * 16 + fr;
      bf[ni] = *(const bf16x8*)&Wl[ch * STEM_WPITCH + r * 32 + fk * 8];
    }
#pragma unroll
    for (int mi = 0; mi < 4; mi++)
#pragma unroll
      for (int ni = 0; ni < 2; ni++)
        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[mi], bf[ni], acc[mi][ni], 0, 0, 0);
  }

  // --- epilogue: y [m][K] + optional BN batch stats ---------------------
  float ssum[2] = {0.f, 0.f}, ssq[2] = {0.f, 0.f};
#pragma unroll
  for (int mi = 0; mi < 4; mi++) {
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      int gn = wc * 32 + ni * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int ml = wr * 64 + mi * 16 + fk * 4 + q;  // D-frag row = fk*4+q
        int hl = ml / wo_pad;
        int wo = ml - hl * wo_pad;
        if (hl < rows_pb && ho0 + hl < p.Ho && wo < p.Wo && gn < p.K) {
          float v = acc[mi][ni][q];
          long gm = (long)(n * p.Ho + ho0 + hl) * p.Wo + wo;
          Y[gm * p.K + gn] = f2b(v);
          if (STATS) {
            ssum[ni] += v;
            ssq[ni] += v * v;
          }
        }
      }
    }
  }
  if (STATS && stats != nullptr) {
#pragma unroll
    for (int ni = 0; ni < 2; ni++) {
      float s = ssum[ni] + __shfl_xor(ssum[ni], 16, 64);
      s += __shfl_xor(s, 32, 64);
      float s2 = ssq[ni] + __shfl_xor(ssq[ni], 16, 64);
      s2 += __shfl_xor(s2, 32, 64);
      int gn = wc * 32 + ni * 16 + fr;
      if (fk == 0 && gn < p.K) {
        atomicAdd(&stats[gn], s);
        atomicAdd(&stats[p.K + gn], s2);
      }
    }
  }
}

static inline bool stem_eligible(const ConvP& p) {
  // measured SLOWER than the generic t128x64 im2col path everywhere
  // (CIFAR 31.5 vs 30.5 us incl. BN; @224 238 vs 206): per-block W LDS
  // staging (64x232 padded image re-built 3.5k times) eats the gather
  // savings.  Kept as an opt-in experiment + measured negative
  // (docs/STATUS.md); default OFF.
  static const int on = (int)env_long("HZ_STEM_DIRECT", 0);
  return on && !taps_clipped(p) && p.C == 3 && p.R == 7 && p.S == 7 &&
         p.str == 2 && p.pad == 3 && p.K <= 64 && p.Wo <= 128;
}

static void launch_stem_conv(const bf16* x, const bf16* w, bf16* y,
                             float* stats, const ConvP& p, hipStream_t st) {
  int wo_pad = ((p.Wo + 15) / 16) * 16;
  int rows_pb = 128 / wo_pad;
  if (rows_pb < 1) rows_pb = 1;
  int bpi = (p.Ho + rows_pb - 1) / rows_pb;
  int amax = 6 * (wo_pad - 1) + 33;
  int xp = 9 + 3 * p.W + 8;
  if (xp < amax) xp = amax;
  xp = ((xp + 7) / 8) * 8;
  int nrows = rows_pb * 2 + 5;
  size_t lds = (size_t)(64 * STEM_WPITCH + nrows * xp) * sizeof(bf16);
  dim3 grid(p.Nb * bpi);
  if (stats != nullptr)
    k_stem_conv<true><<<grid, 256, lds, st>>>(x, w, y, stats, p, rows_pb,
                                              wo_pad, xp, bpi);
  else
    k_stem_conv<false><<<grid, 256, lds, st>>>(x, w, y, nullptr, p, rows_pb,
                                               wo_pad, xp, bpi);
}

// Throughput-tile selection: the biggest block tile whose grid still
// fills the 256 CUs (HZ_TILE_FILL, default 192 blocks).  CIFAR-shape
// grids stay on the latency-optimized 64×64 tile; ImageNet-shaped convs
// (ResNet50@224 etc.) move to 128×64 / 128×128 where each wave issues
// 2–4× the MFMAs per LDS fragment read.
static inline int pick_tile_env(int M, int N, int fill, int m_min,
                                int m_min256) {
  if (M < m_min) return 0;
  if (M >= m_min256 && N < 128
      && (long)cdiv_h(M, 256) * cdiv_h(N, 64) >= fill)
    return 3;
  if (N >= 128 && (long)cdiv_h(M, 128) * cdiv_h(N, 128) >= fill) return 2;
  if ((long)cdiv_h(M, 128) * cdiv_h(N, 64) >= fill) return 1;
  return 0;
}

// dgrad has its own thresholds: no stats epilogue and an RSCK B-gather,
// so the fwd-measured floors need not match (HZ_TILE_*_DG)
static inline int pick_tile_dgrad(int M, int N) {
  static const int fill = (int)env_long("HZ_TILE_FILL_DG", 192);
  static const int m_min = (int)env_long("HZ_TILE_M_MIN_DG", 16384);
  static const int m256 = (int)env_long("HZ_TILE_M256_DG", 65536);
  return pick_tile_env(M, N, fill, m_min, m256);
}

static inline int pick_tile(int M, int N) {
  static const int fill = (int)env_long("HZ_TILE_FILL", 192);
  // measured (conv sweep, r50@224 bs=32): the 128-row tiles win
  // from M≈25k up (+30-60% fwd) but lose ~20% at M≈6k even when the
  // grid-fill bound is met — keep a hard M floor
  static const int m_min = (int)env_long("HZ_TILE_M_MIN", 16384);
  // 256x64 (tile 3): very-large-M thin-N shapes (stem/layer1 @224)
  static const int m_min256 = (int)env_long("HZ_TILE_M256", 65536);
  return pick_tile_env(M, N, fill, m_min, m_min256);
}

// Non-split forward (bf16 out + fused stats).
extern "C" void launch_conv_fwd(const void* x, const void* w, void* y,
                                float* stats, ConvP p, hipStream_t st) {
  if (stem_eligible(p)) {
    launch_stem_conv((const bf16*)x, (const bf16*)w, (bf16*)y, stats, p,
                     st);
    return;
  }
  bool vec = (p.C % 8) == 0 && (p.Kd % 8) == 0;
  bool s = stats != nullptr;
  auto A = (const bf16*)x;
  auto B = (const bf16*)w;
  auto Y = (bf16*)y;
  MagicP mg = make_magic(p, 1);
  int tile = conv_tile(p);
#define CASE_T(VA, VB, ST, TM, TN, CL)                                    \
  k_conv_mfma<1, VA, VB, ST, false, TM, TN, false, CL>                    \
      <<<grid, 256, 0, st>>>(A, B, Y, nullptr, stats, p, mg, p.K, 0, 0)
#define DISPATCH(TM, TN, CL)                                              \
  do {                                                                    \
    dim3 grid(cdiv_h(p.K, TN), cdiv_h(p.M, TM));                          \
    if (vec && s) CASE_T(true, true, true, TM, TN, CL);                   \
    else if (vec) CASE_T(true, true, false, TM, TN, CL);                  \
    else if (s) CASE_T(false, false, true, TM, TN, CL);                   \
    else CASE_T(false, false, false, TM, TN, CL);                         \
  } while (0)
  if (tile == 3) DISPATCH(256, 64, false);
  else if (tile == 2) DISPATCH(128, 128, false);
  else if (tile == 1) DISPATCH(128, 64, false);
  else if (taps_clipped(p)) DISPATCH(64, 64, true);
  else DISPATCH(64, 64, false);
#undef DISPATCH
#undef CASE_T
}

// Split-K forward: f32 atomic partials into ws (pre-zeroed [M][K]).
extern "C" void launch_conv_fwd_splitk(const void* x, const void* w,
                                       float* ws, ConvP p, int splitk,
                                       hipStream_t st) {
  int kchunk = cdiv_h(cdiv_h(p.Kd, splitk), 32) * 32;
  splitk = cdiv_h(p.Kd, kchunk);
  bool vec = (p.C % 8) == 0 && (p.Kd % 8) == 0;
  auto A = (const bf16*)x;
  auto B = (const bf16*)w;
  MagicP mg = make_magic(p, 1);
  // fill-split shapes keep their throughput tile; the classic small-M
  // split shapes pick tile 0 (64x64) as before
  int tile = conv_tile(p);
#define SK_T(VA, VB, TM, TN, CL)                                        \
  k_conv_mfma<1, VA, VB, false, true, TM, TN, false, CL>                \
      <<<grid, 256, 0, st>>>(A, B, nullptr, ws, nullptr, p, mg, p.K,    \
                             kchunk, 0)
#define DISPATCH(TM, TN, CL)                                            \
  do {                                                                  \
    dim3 grid(cdiv_h(p.K, TN), cdiv_h(p.M, TM), splitk);                \
    if (vec) SK_T(true, true, TM, TN, CL);                              \
    else SK_T(false, false, TM, TN, CL);                                \
  } while (0)
  if (tile == 3) DISPATCH(256, 64, false);
  else if (tile == 2) DISPATCH(128, 128, false);
  else if (tile == 1) DISPATCH(128, 64, false);
  else if (taps_clipped(p)) DISPATCH(64, 64, true);
  else DISPATCH(64, 64, false);
#undef DISPATCH
#undef SK_T
}

// KRSC-direct dgrad, one tile class: the split / non-split form and the
// vector flags (A gathers vec8 along ko, B along c).
template <int TM, int TN, bool CL = false>
static void dgrad_krsc_t(const bf16* A, const bf16* B, bf16* dx, float* ws,
                         bool split, int splitk, int kchunk, const ConvP& p,
                         const MagicP& mg, int accum, hipStream_t st) {
  dim3 grid(cdiv_h(p.C, TN), cdiv_h(p.M, TM), split ? splitk : 1);
  const bool va = (p.K % 8) == 0, vb = (p.C % 8) == 0;
#define KRSC_T(VA, VB)                                                      \
  do {                                                                      \
    if (split)                                                              \
      k_conv_mfma<2, VA, VB, false, true, TM, TN, true, CL>                 \
          <<<grid, 256, 0, st>>>(A, B, nullptr, ws, nullptr, p, mg, p.C,    \
                                 kchunk, 0);                                \
    else                                                                    \
      k_conv_mfma<2, VA, VB, false, false, TM, TN, true, CL>                \
          <<<grid, 256, 0, st>>>(A, B, dx, nullptr, nullptr, p, mg, p.C, 0, \
                                 accum);                                    \
  } while (0)
  if (va && vb) KRSC_T(true, true);
  else if (va) KRSC_T(true, false);
  else if (vb) KRSC_T(false, true);
  else KRSC_T(false, false);
#undef KRSC_T
}

// w_layout: DGRAD_W_RSCK — `w` is the permuted RSCK image (MODE 2 as ever);
// DGRAD_W_KRSC — `w` is the KRSC weight itself (transposed-read B path).
// Tile and split selection do not depend on the layout.
extern "C" void launch_conv_dgrad(const void* dz, const void* w, void* dx,
                                  float* ws, int splitk, ConvP p, int accum,
                                  int w_layout, hipStream_t st) {
  // p here: M = Nb*H*W, Kd = R*S*K, output channels = C
  bool vec = (p.K % 8) == 0;
  auto A = (const bf16*)dz;
  auto B = (const bf16*)w;
  if (w_layout == DGRAD_W_KRSC) {
    const bool split = splitk > 1;
    int kchunk = 0;
    if (split) {
      kchunk = cdiv_h(cdiv_h(p.Kd, splitk), 32) * 32;
      splitk = cdiv_h(p.Kd, kchunk);
    }
    MagicP mg = make_magic(p, 2);
    int tile = conv_tile_dgrad(p);
#define DISPATCH(TM, TN, CL)                                             \
  dgrad_krsc_t<TM, TN, CL>(A, B, (bf16*)dx, ws, split, splitk, kchunk, p, \
                           mg, accum, st)
    if (tile == 3) DISPATCH(256, 64, false);
    else if (tile == 2) DISPATCH(128, 128, false);
    else if (tile == 1) DISPATCH(128, 64, false);
    else if (taps_clipped(p)) DISPATCH(64, 64, true);
    else DISPATCH(64, 64, false);
#undef DISPATCH
    return;
  }
  if (splitk > 1) {
    int kchunk = cdiv_h(cdiv_h(p.Kd, splitk), 32) * 32;
    splitk = cdiv_h(p.Kd, kchunk);
    MagicP mg = make_magic(p, 2);
    int tile = conv_tile_dgrad(p);
#define SKD_T(VA, VB, TM, TN, CL)                                       \
  k_conv_mfma<2, VA, VB, false, true, TM, TN, false, CL>                \
      <<<grid, 256, 0, st>>>(A, B, nullptr, ws, nullptr, p, mg, p.C,    \
                             kchunk, 0)
#define DISPATCH(TM, TN, CL)                                            \
  do {                                                                  \
    dim3 grid(cdiv_h(p.C, TN), cdiv_h(p.M, TM), splitk);                \
    if (vec) SKD_T(true, true, TM, TN, CL);                             \
    else SKD_T(false, false, TM, TN, CL);                               \
  } while (0)
    if (tile == 3) DISPATCH(256, 64, false);
    else if (tile == 2) DISPATCH(128, 128, false);
    else if (tile == 1) DISPATCH(128, 64, false);
    else if (taps_clipped(p)) DISPATCH(64, 64, true);
    else DISPATCH(64, 64, false);
#undef DISPATCH
#undef SKD_T
  } else {
    MagicP mg = make_magic(p, 2);
    int tile = conv_tile_dgrad(p);
#define DGRAD_T(VA, VB, TM, TN, CL)                                     \
  k_conv_mfma<2, VA, VB, false, false, TM, TN, false, CL>               \
      <<<grid, 256, 0, st>>>(A, B, (bf16*)dx, nullptr, nullptr, p, mg,  \
                             p.C, 0, accum)
#define DISPATCH(TM, TN, CL)                                            \
  do {                                                                  \
    dim3 grid(cdiv_h(p.C, TN), cdiv_h(p.M, TM));                        \
    if (vec) DGRAD_T(true, true, TM, TN, CL);                           \
    else DGRAD_T(false, false, TM, TN, CL);                             \
  } while (0)
    if (tile == 3) DISPATCH(256, 64, false);
    else if (tile == 2) DISPATCH(128, 128, false);
    else if (tile == 1) DISPATCH(128, 64, false);
    else if (taps_clipped(p)) DISPATCH(64, 64, true);
    else DISPATCH(64, 64, false);
#undef DISPATCH
#undef DGRAD_T
  }
}

extern "C" void launch_gemm_bf16(const void* a, const void* b, void* c, int M,
                                 int N, int K, hipStream_t st) {
  ConvP p{};
  p.M = M;
  p.Kd = K;
  dim3 grid(cdiv_h(N, 64), cdiv_h(M, 64));
  bool vec = (K % 8) == 0;
  MagicP mg{};
  if (vec)
    k_conv_mfma<0, true, true, false, false>
        <<<grid, 256, 0, st>>>((const bf16*)a, (const bf16*)b, (bf16*)c,
                               nullptr, nullptr, p, mg, N, 0, 0);
  else
    k_conv_mfma<0, false, false, false, false>
        <<<grid, 256, 0, st>>>((const bf16*)a, (const bf16*)b, (bf16*)c,
                               nullptr, nullptr, p, mg, N, 0, 0);
}

// tile class per task batch: tx/ty counted in (tk3, tko)-wide tiles by
// the caller.  128-wide k3 halves Dz re-reads; 128-wide ko halves X
// re-reads; both double the MFMA per staging write.
template <bool TR>
static void wgrad_batched_tr(const WgradBatchArgs& a, int blocks, int tk3,
                             int tko, hipStream_t st) {
  if (tk3 == 128 && tko == 128)
    k_wgrad_batched<128, 128, TR><<<blocks, 256, 0, st>>>(a);
  else if (tk3 == 128)
    k_wgrad_batched<128, 64, TR><<<blocks, 256, 0, st>>>(a);
  else if (tko == 128)
    k_wgrad_batched<64, 128, TR><<<blocks, 256, 0, st>>>(a);
  else
    k_wgrad_batched<64, 64, TR><<<blocks, 256, 0, st>>>(a);
}

// tr: row-major images + transposed reads (nonzero) or the transposed-scatter
// body (0).
extern "C" void launch_wgrad_batched_t(const WgradBatchArgs* args, int blocks,
                                       int tk3, int tko, int tr,
                                       hipStream_t st) {
  if (blocks <= 0) return;
  if (tr) wgrad_batched_tr<true>(*args, blocks, tk3, tko, st);
  else wgrad_batched_tr<false>(*args, blocks, tk3, tko, st);
}

extern "C" void launch_wgrad_reduce_batched(const WredBatchArgs* args,
                                            int blocks, hipStream_t st) {
  if (blocks > 0) k_wgrad_reduce_batched<<<blocks, 256, 0, st>>>(*args);
}

extern "C" int wgrad_msplit(ConvP p) {
  int tiles = cdiv_h(p.Kd, 64) * cdiv_h(p.K, 64);
  int msplit = max(1, min(cdiv_h(p.M, 32), 512 / max(1, tiles)));
  int mchunk = cdiv_h(cdiv_h(p.M, msplit), 32) * 32;
  return cdiv_h(p.M, mchunk);
}

// ws: per-split slab workspace [msplit][K][Kd] f32 (only read/written when
// msplit > 1); dw must be pre-zeroed (direct-grad .grad view or fresh).
extern "C" void launch_wgrad(const void* x, const void* dz, float* dw,
                             float* ws, ConvP p, int tr, hipStream_t st) {
  int msplit = wgrad_msplit(p);
  int mchunk = cdiv_h(cdiv_h(p.M, msplit), 32) * 32;
  dim3 grid(cdiv_h(p.Kd, 64), cdiv_h(p.K, 64), msplit);
  bool vec = (p.C % 8) == 0;
  float* out = msplit > 1 ? ws : dw;
  MagicP mg = make_magic(p, 1);
#define WGRAD_T(VA, TR, CL)                                           \
  k_wgrad<VA, TR, CL><<<grid, 256, 0, st>>>(                          \
      (const bf16*)x, (const bf16*)dz, out, p, mg, p.K, mchunk)
#define DISPATCH(TR, CL)            \
  do {                              \
    if (vec) WGRAD_T(true, TR, CL); \
    else WGRAD_T(false, TR, CL);    \
  } while (0)
  if (taps_clipped(p)) {
    if (tr) DISPATCH(true, true);
    else DISPATCH(false, true);
  } else if (tr) DISPATCH(true, false);
  else DISPATCH(false, false);
#undef DISPATCH
#undef WGRAD_T
  if (msplit > 1) {
    WredTask t{};
    t.ws = ws;
    t.dW = dw;
    t.n = (long)p.K * p.Kd;
    t.msplit = msplit;
    wred_set_window(&t, p);
    int blocks = (int)max(1L, min((t.n / 4 + 255) / 256, (long)1024));
    k_wgrad_reduce<<<blocks, 256, 0, st>>>(t);
  }
}
