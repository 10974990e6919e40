// Folded-BatchNorm inference kernels for gfx950 (MI355X, CDNA4).
//
// In eval mode BatchNorm is a per-channel affine map, so a conv+BN+act module
// is one kernel:
//   y[m,k] = act( acc[m,k]·scale[k] + bias[k] (+ res[m,k]) )
// with scale = γ/sqrt(var+eps), bias = β − mean·scale folded on the host
// (models/infer.py).  No convout, no statistics, no atomics, no workspace:
// one launch per conv, the same result with the deterministic switch on or
// off.
//
// k_conv_infer: dense implicit GEMM over NHWC x and KRSC w on
// mfma_f32_16x16x32_bf16, as a TRANSPOSED product: the weights are the MFMA
// A operand (rows = output channels) and the pixels the B operand (columns =
// pixels).  The D fragment of lane (fr = lane & 15, fk = lane >> 4) is then
//   D[q] = channel 4·fk + q of pixel fr,   q = 0..3
// four CONSECUTIVE output channels of one pixel: the epilogue reads scale and
// bias as float4, the residual as 8 bytes and writes y as 8 bytes (the
// training kernel's fragment is four pixels of one channel: four 2-byte
// accesses K elements apart).
//
// Two forms, picked per conv (infer_pick_wsplit):
//  * tile form: 64 pixels × 64 channels per block, the four waves in 2×2,
//    double-buffered LDS, one barrier per 32-wide K-step;
//  * wave-split form (small M, long K): 32 pixels × 32 channels per block and
//    each wave takes a contiguous quarter of the K loop in whole K-steps, on
//    its own double-buffered pair of 32×32 operand tiles.  The four partial
//    tiles meet in LDS and wave w finishes fragment w, summing the partials
//    in wave order 0,1,2,3 — a fixed order, so the result does not depend on
//    scheduling.  One launch, no slab workspace.
//
// Zero-fill rule: pixels ≥ M, k ≥ the wave's K end, channels ≥ K and padding
// taps are ZEROS in LDS, never masked lanes; control flow around the MFMAs
// and barriers is block-uniform.
//
// k_dw_infer: the depthwise stencil with the same epilogue.
#include "common.h"

#define ILDA 40  // 32 + 8 pad; row stride 80 B (the k_conv_mfma image)

union V4 {
  uint2 u;
  bf16 e[4];
};

DEV float act_apply(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return fminf(fmaxf(v, 0.f), 6.f);
  return v;
}

// --------------------------------------------------------------- gathers --
// Forward only, so the pixel of a staging row is decomposed ONCE, before the
// K loop; a K-step decomposes its k once per thread and shares (r, s, c)
// between the x and the w gather.  The tap window (launch.h, clip_taps) moves
// the patch origin by (r0, s0), folded into the hoisted pixel, and addresses
// w through the full Rf×Sf filter (CLIP).
struct PixP {
  int n, hi0, wi0;  // image, input coordinates of window tap (0, 0)
  bool ok;          // m < M
};

DEV PixP pix_of(const ConvP& p, const MagicP& mg, unsigned m) {
  PixP q;
  q.ok = m < (unsigned)p.M;
  const unsigned mm = q.ok ? m : 0u;
  unsigned n = fdiv(mm, mg, 0), hw = fmod(mm, n, mg, 0);
  unsigned ho = fdiv(hw, mg, 1), wo = fmod(hw, ho, mg, 1);
  q.n = (int)n;
  q.hi0 = (int)ho * p.str - p.pad + p.r0;
  q.wi0 = (int)wo * p.str - p.pad + p.s0;
  return q;
}

struct KPos {
  int r, s, c;
};

DEV KPos kpos(const MagicP& mg, int k) {
  unsigned r = fdiv(k, mg, 2), rm = fmod(k, r, mg, 2);
  unsigned s = fdiv(rm, mg, 3), c = fmod(rm, s, mg, 3);
  return KPos{(int)r, (int)s, (int)c};
}

// eight consecutive k of one pixel's patch.  VEC: C % 8 == 0, so they share
// the tap and are one 16-byte load; otherwise (the C = 3 stem) eight scalar
// loads with an incremental carry through (c, s, r).
template <bool VEC>
DEV V8 gather_x(const bf16* __restrict__ x, const ConvP& p, const PixP& q,
                const KPos& kp, int k, int kend) {
  V8 v;
  if (VEC) {
    const int hi = q.hi0 + kp.r, wi = q.wi0 + kp.s;
    const bool ok = q.ok & (k < kend) & (hi >= 0) & (hi < p.H) & (wi >= 0) &
                    (wi < p.W);
    if (ok)
      v.u = *(const uint4*)(x + ((long)((q.n * p.H + hi) * p.W + wi) * p.C +
                                 kp.c));
    else
      v.u = uint4{0, 0, 0, 0};
  } else {
    int r = kp.r, s = kp.s, c = kp.c;
    int hi = q.hi0 + r, wi = q.wi0 + s;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const bool ok = q.ok && k + e < kend && hi >= 0 && hi < p.H &&
                      wi >= 0 && wi < p.W;
      v.e[e] = ok ? x[(long)((q.n * p.H + hi) * p.W + wi) * p.C + c]
                  : (bf16)0.f;
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
  }
  return v;
}

// eight consecutive k of filter `ko`.  Window element k lies at
//   ko·KdF + org + k + r·skip
// of the filter as stored (KdF = Rf·Sf·C, org = (r0·Sf + s0)·C, skip =
// (Sf − S)·C); unclipped that is ko·Kd + k and needs no decomposition.
template <bool VEC, bool CLIP>
DEV V8 gather_w(const bf16* __restrict__ w, const ConvP& p, int ko,
                const KPos& kp, int k, int kend) {
  V8 v;
  const bool rok = ko < p.K;
  const long row = (long)ko * (CLIP ? p.Rf * p.Sf * p.C : p.Kd);
  const int org = CLIP ? (p.r0 * p.Sf + p.s0) * p.C : 0;
  const int skip = CLIP ? (p.Sf - p.S) * p.C : 0;
  if (VEC) {
    if (rok && k < kend)
      v.u = *(const uint4*)(w + row + org + k + (CLIP ? kp.r * skip : 0));
    else
      v.u = uint4{0, 0, 0, 0};
  } else {
    int r = kp.r, s = kp.s, c = kp.c;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const bool ok = rok && k + e < kend;
      v.e[e] = ok ? w[row + org + k + e + (CLIP ? r * skip : 0)] : (bf16)0.f;
      if (CLIP && ++c == p.C) {
        c = 0;
        if (++s == p.S) {
          s = 0;
          ++r;
        }
      }
    }
  }
  return v;
}

// -------------------------------------------------------------- epilogue --
// v = channels gk .. gk+3 of pixel gm.  EPI4: K % 4 == 0 and every pointer
// aligned for the vector accesses (the launcher checks), so gk + 3 < K.
template <bool EPI4>
DEV void epi_store(f32x4 v, unsigned gm, int gk, const ConvP& p,
                   const float* __restrict__ scale,
                   const float* __restrict__ bias,
                   const bf16* __restrict__ res, bf16* __restrict__ y,
                   int act) {
  if (gm >= (unsigned)p.M || gk >= p.K) return;
  const long o = (long)gm * p.K + gk;
  if (EPI4) {
    const float4 sc = *(const float4*)(scale + gk);
    const float4 bi = *(const float4*)(bias + gk);
    float t[4] = {fmaf(v[0], sc.x, bi.x), fmaf(v[1], sc.y, bi.y),
                  fmaf(v[2], sc.z, bi.z), fmaf(v[3], sc.w, bi.w)};
    if (res != nullptr) {
      V4 r;
      r.u = *(const uint2*)(res + o);
#pragma unroll
      for (int q = 0; q < 4; q++) t[q] += b2f(r.e[q]);
    }
    V4 out;
#pragma unroll
    for (int q = 0; q < 4; q++) out.e[q] = f2b(act_apply(t[q], act));
    *(uint2*)(y + o) = out.u;
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      if (gk + q < p.K) {
        float t = fmaf(v[q], scale[gk + q], bias[gk + q]);
        if (res != nullptr) t += b2f(res[o + q]);
        y[o + q] = f2b(act_apply(t, act));
      }
    }
  }
}

// ------------------------------------------------------------ conv kernel --
// LDS, in bf16 elements (TILE = rows × ILDA):
//   tile form   [buf 2][X 64 rows | W 64 rows]                 20 KB
//   wave split  [wave 4][buf 2][X 32 rows | W 32 rows]          40 KB
//               and, after the K loop, the f32 partials
//               [wave 4][fragment 4][lane 64] float4            16 KB
// A thread stages column chunk (tid & 3)·8 of row tid >> 2 (tile form) or of
// rows (lane >> 2) and (lane >> 2) + 16 of its wave's tiles (wave split), for
// x and w alike, so one k decomposition serves all of a thread's gathers.
template <bool WS, bool VEC, bool CLIP, bool EPI4>
__global__ __launch_bounds__(256) void k_conv_infer(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const bf16* __restrict__ res, bf16* __restrict__ y, ConvP p, MagicP mg,
    int act) {
  constexpr int TR = WS ? 32 : 64;   // rows of an operand tile
  constexpr int NCH = WS ? 2 : 1;    // staging chunks per thread and operand
  constexpr int TILE = TR * ILDA;
  __shared__ __attribute__((aligned(16))) bf16 sm[(WS ? 16 : 4) * TILE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
  const unsigned m0 = blockIdx.x * (unsigned)TR;
  const int c0 = blockIdx.y * TR;

  // K range of this wave: the whole loop, or its quarter in whole K-steps.
  // nst is block-uniform; a quarter that ends early (or is empty) stages
  // zeros for its remaining steps.
  const int nsteps = (p.Kd + 31) >> 5;
  const int nst = WS ? (nsteps + 3) >> 2 : nsteps;
  const int kbeg = WS ? wave * nst * 32 : 0;
  const int kend = WS ? min(p.Kd, kbeg + nst * 32) : p.Kd;

  bf16* reg = sm + (WS ? wave * 4 * TILE : 0);
  const int scol = (tid & 3) * 8;
  int srow[NCH], ko[NCH];
  PixP px[NCH];
#pragma unroll
  for (int j = 0; j < NCH; j++) {
    srow[j] = WS ? j * 16 + (lane >> 2) : tid >> 2;
    px[j] = pix_of(p, mg, m0 + (unsigned)srow[j]);
    ko[j] = c0 + srow[j];
  }

  V8 xn[NCH], wn[NCH];
  auto load = [&](int k0) {
    const int k = k0 + scol;
    const KPos kp = kpos(mg, k);
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      xn[j] = gather_x<VEC>(x, p, px[j], kp, k, kend);
      wn[j] = gather_w<VEC, CLIP>(w, p, ko[j], kp, k, kend);
    }
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      *(V8*)&reg[b * 2 * TILE + srow[j] * ILDA + scol] = xn[j];
      *(V8*)&reg[b * 2 * TILE + TILE + srow[j] * ILDA + scol] = wn[j];
    }
  };

  f32x4 acc[2][2] = {};  // [channel fragment][pixel fragment]

  // prologue: step 0 -> LDS[0]; step 1 -> registers
  load(kbeg);
  stage(0);
  if (1 < nst) load(kbeg + 32);
  __syncthreads();

  int buf = 0;
  for (int i = 0; i < nst; i++) {
    // step i+1 from registers into the other buffer (its readers passed the
    // previous barrier), then step i+2's loads go in flight
    if (i + 1 < nst) {
      stage(buf ^ 1);
      if (i + 2 < nst) load(kbeg + (i + 2) * 32);
    }
    const bf16* xs = reg + buf * 2 * TILE + (WS ? 0 : wr * 32) * ILDA;
    const bf16* ws = reg + buf * 2 * TILE + TILE + (WS ? 0 : wc * 32) * ILDA;
    bf16x8 wf[2], xf[2];
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
      wf[ci] = *(const bf16x8*)&ws[(ci * 16 + fr) * ILDA + fk * 8];
#pragma unroll
    for (int pi = 0; pi < 2; pi++)
      xf[pi] = *(const bf16x8*)&xs[(pi * 16 + fr) * ILDA + fk * 8];
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
      for (int pi = 0; pi < 2; pi++)
        acc[ci][pi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf[ci], xf[pi], acc[ci][pi], 0, 0, 0);
    buf ^= 1;
    __syncthreads();
  }

  if (WS) {
    // the loop's last barrier freed the staging LDS: partials in, barrier,
    // wave w sums fragment w in wave order and runs its epilogue
    f32x4* red = (f32x4*)sm;
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
      for (int pi = 0; pi < 2; pi++)
        red[(wave * 4 + ci * 2 + pi) * 64 + lane] = acc[ci][pi];
    __syncthreads();
    f32x4 t = red[wave * 64 + lane];
#pragma unroll
    for (int u = 1; u < 4; u++) t += red[(u * 4 + wave) * 64 + lane];
    epi_store<EPI4>(t, m0 + (unsigned)(wc * 16 + fr), c0 + wr * 16 + fk * 4,
                    p, scale, bias, res, y, act);
  } else {
#pragma unroll
    for (int ci = 0; ci < 2; ci++)
#pragma unroll
      for (int pi = 0; pi < 2; pi++)
        epi_store<EPI4>(acc[ci][pi],
                        m0 + (unsigned)(wr * 32 + pi * 16 + fr),
                        c0 + wc * 32 + ci * 16 + fk * 4, p, scale, bias, res,
                        y, act);
  }
}

// ------------------------------------------------------- depthwise kernel --
// Channel c maps to itself: a per-channel stencil, bandwidth-bound, no MFMA.
// A thread owns one channel group (8 channels, 16-byte accesses, when VEC;
// else one channel) for its whole life and walks pixels: consecutive threads
// are consecutive groups of one pixel, then the next pixel, so every access
// is a contiguous run; the grid covers `mstride` whole pixels per pass and
// the few threads past them idle.  The group's taps (KS×KS, as packed bf16),
// scale and bias are loaded once into registers; KS = 0 is the generic
// filter, which reads its taps through the cache instead.  The output pixel
// is decomposed once per vector.
template <int KS, bool VEC>
__global__ __launch_bounds__(256) void k_dw_infer(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ scale, const float* __restrict__ bias,
    const bf16* __restrict__ res, bf16* __restrict__ y, int H, int W, int C,
    int Ho, int Wo, int R, int S, int str, int pad, int M, int CG,
    int mstride, int act) {
  constexpr int CH = VEC ? 8 : 1;
  constexpr int NT = KS ? KS * KS : 1;
  const unsigned gt = blockIdx.x * 256u + threadIdx.x;
  if (gt >= (unsigned)mstride * (unsigned)CG) return;  // no barrier below
  const int c = (int)(gt % (unsigned)CG) * CH;

  V8 wv[NT];
  float wf[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    wv[t].u = uint4{0, 0, 0, 0};
    wf[t] = 0.f;
    if (KS && VEC) wv[t].u = *(const uint4*)(w + (long)t * C + c);
    if (KS && !VEC) wf[t] = b2f(w[(long)t * C + c]);
  }
  float sc[CH], bi[CH];
#pragma unroll
  for (int e = 0; e < CH; e++) {
    sc[e] = scale[c + e];
    bi[e] = bias[c + e];
  }

  for (int m = (int)(gt / (unsigned)CG); m < M; m += mstride) {
    const int n = m / (Ho * Wo), hw = m - n * (Ho * Wo);
    const int ho = hw / Wo, wo = hw - ho * Wo;
    const int hi0 = ho * str - pad, wi0 = wo * str - pad;
    float acc[CH];
#pragma unroll
    for (int e = 0; e < CH; e++) acc[e] = 0.f;
    // one tap: x[n, hi, wi, c..] times tap t of this group
    auto tap = [&](int hi, int wi, const V8& tv, float tf) {
      if (hi < 0 || hi >= H || wi < 0 || wi >= W) return;
      const long xi = ((long)(n * H + hi) * W + wi) * C + c;
      if (VEC) {
        V8 xv;
        xv.u = *(const uint4*)(x + xi);
#pragma unroll
        for (int e = 0; e < 8; e++)
          acc[e] = fmaf(b2f(xv.e[e]), b2f(tv.e[e]), acc[e]);
      } else {
        acc[0] = fmaf(b2f(x[xi]), tf, acc[0]);
      }
    };
    if (KS) {
#pragma unroll
      for (int r = 0; r < KS; r++)
#pragma unroll
        for (int s = 0; s < KS; s++)
          tap(hi0 + r, wi0 + s, wv[r * KS + s], wf[r * KS + s]);
    } else {
      for (int r = 0; r < R; r++)
        for (int s = 0; s < S; s++) {
          V8 tv;
          tv.u = uint4{0, 0, 0, 0};
          float tf = 0.f;
          const long wo_ = (long)(r * S + s) * C + c;
          if (VEC) tv.u = *(const uint4*)(w + wo_);
          else tf = b2f(w[wo_]);
          tap(hi0 + r, wi0 + s, tv, tf);
        }
    }
    const long o = (long)m * C + c;
    if (VEC) {
      V8 rv, out;
      if (res != nullptr) rv.u = *(const uint4*)(res + o);
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float t = fmaf(acc[e], sc[e], bi[e]);
        if (res != nullptr) t += b2f(rv.e[e]);
        out.e[e] = f2b(act_apply(t, act));
      }
      *(uint4*)(y + o) = out.u;
    } else {
      float t = fmaf(acc[0], sc[0], bi[0]);
      if (res != nullptr) t += b2f(res[o]);
      y[o] = f2b(act_apply(t, act));
    }
  }
}

// ============================================================== launchers ==
static long g_infer_tile = 0, g_infer_ws = 0, g_infer_dw = 0;
// -1 auto, 0 never, 1 always (HZ_INFER_WSPLIT at load; docs/TUNING.md)
static int g_infer_wsplit = (int)env_long("HZ_INFER_WSPLIT", -1);

// Kd floor of the automatic wave split (HZ_INFER_WSPLIT_KD at load; the
// sweep behind the default is in docs/TUNING.md).
static const int g_infer_wsplit_kd =
    (int)env_long("HZ_INFER_WSPLIT_KD", 32);

static inline bool al(const void* ptr, unsigned n) {
  return ((size_t)ptr & (n - 1)) == 0;
}

template <bool WS, bool VEC, bool CLIP>
static void conv_infer_go(bool epi4, dim3 grid, const bf16* x, const bf16* w,
                          const float* scale, const float* bias,
                          const bf16* res, bf16* y, const ConvP& p,
                          const MagicP& mg, int act, hipStream_t st) {
  if (epi4)
    k_conv_infer<WS, VEC, CLIP, true>
        <<<grid, 256, 0, st>>>(x, w, scale, bias, res, y, p, mg, act);
  else
    k_conv_infer<WS, VEC, CLIP, false>
        <<<grid, 256, 0, st>>>(x, w, scale, bias, res, y, p, mg, act);
}

extern "C" {

void set_infer_wsplit(int mode) {
  g_infer_wsplit = mode < 0 ? -1 : (mode > 0 ? 1 : 0);
}
int infer_wsplit() { return g_infer_wsplit; }

void infer_launch_counts(long* tile, long* wsplit, long* dw) {
  *tile = g_infer_tile;
  *wsplit = g_infer_ws;
  *dw = g_infer_dw;
}

// 1 = wave-split form.  Auto: the 64×64 tiling leaves CUs idle (fewer blocks
// than the 256 CUs) and the live K loop is long enough to quarter.
int infer_pick_wsplit(ConvP p) {
  if (g_infer_wsplit >= 0) return g_infer_wsplit;
  const long tiles = ((long)p.M + 63) / 64 * ((p.K + 63) / 64);
  return tiles < 256 && p.Kd >= g_infer_wsplit_kd;
}

void launch_conv_infer(const void* x, const void* w, const float* scale,
                       const float* bias, const void* res, void* y, ConvP p,
                       int act, hipStream_t st) {
  const MagicP mg = make_magic(p, 1);
  const bool ws = infer_pick_wsplit(p) != 0;
  const bool vec = p.C % 8 == 0 && al(x, 16) && al(w, 16);
  const bool clip = taps_clipped(p);
  const bool epi4 = p.K % 4 == 0 && al(y, 8) && al(res, 8) && al(scale, 16) &&
                    al(bias, 16);
  const int tr = ws ? 32 : 64;
  dim3 grid((unsigned)(((long)p.M + tr - 1) / tr), (p.K + tr - 1) / tr);
#define GO(WS, VEC, CLIP)                                                   \
  conv_infer_go<WS, VEC, CLIP>(epi4, grid, (const bf16*)x, (const bf16*)w,  \
                               scale, bias, (const bf16*)res, (bf16*)y, p,  \
                               mg, act, st)
  if (ws) {
    if (vec) { if (clip) GO(true, true, true); else GO(true, true, false); }
    else { if (clip) GO(true, false, true); else GO(true, false, false); }
    g_infer_ws++;
  } else {
    if (vec) { if (clip) GO(false, true, true); else GO(false, true, false); }
    else { if (clip) GO(false, false, true); else GO(false, false, false); }
    g_infer_tile++;
  }
#undef GO
}

void launch_dw_infer(const void* x, const void* w, const float* scale,
                     const float* bias, const void* res, void* y, int Nb,
                     int H, int W, int C, int Ho, int Wo, int R, int S,
                     int str, int pad, int act, hipStream_t st) {
  const bool vec = C % 8 == 0 && al(x, 16) && al(w, 16) && al(y, 16) &&
                   al(res, 16);
  const int M = Nb * Ho * Wo;
  const int CG = vec ? C / 8 : C;
  const long total = (long)M * CG;
  long blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks * 256 < CG) blocks = (CG + 255) / 256;
  const int mstride = (int)(blocks * 256 / CG);
  const int ks = (R == S && (R == 3 || R == 5)) ? R : 0;
#define GO(KS, VEC)                                                        \
  k_dw_infer<KS, VEC><<<(unsigned)blocks, 256, 0, st>>>(                   \
      (const bf16*)x, (const bf16*)w, scale, bias, (const bf16*)res,       \
      (bf16*)y, H, W, C, Ho, Wo, R, S, str, pad, M, CG, mstride, act)
  if (vec) {
    if (ks == 3) GO(3, true); else if (ks == 5) GO(5, true); else GO(0, true);
  } else {
    if (ks == 3) GO(3, false);
    else if (ks == 5) GO(5, false);
    else GO(0, false);
  }
#undef GO
  g_infer_dw++;
}

}  // extern "C"
