// Grouped convolution for gfx950 (MI355X, CDNA4), 1 < groups < C: forward,
// data gradient and weight gradient on the bf16 16×16×32 MFMA.  The ResNeXt
// 3×3.  docs/KERNELS.md, "Grouped convolution".
//
// Domain (bind.cpp refuses the rest): Cg == Kg in {4, 8, 16, 32}, so C == K;
// square R in {1, 3}; stride in {1, 2}; C % 16 == 0.  Activations bf16 NHWC,
// weight bf16 [K][R][R][Cg].
//
// Weight-stationary block-diagonal slab.  The unit of work is a slab of 16
// output columns n0 .. n0+15 (output channels in forward, input channels in
// dgrad).  The channels it contracts over are contiguous in NHWC: k0 =
// (n0 / Cg)·Cg and CS = max(16, Cg) of them — 16/Cg whole groups at Cg ≤ 16,
// the slab's own group at Cg = 32.  Its GEMM is [M × T·CS]·[T·CS × 16] with
// T = R·R taps and k = tap·CS + c; B[k][n] is the weight inside the diagonal
// block of column n's group and an exact zero outside it.  The B image is
// ceil(T·CS/32) fragments (1, 5 or 9), built once per block and kept in
// registers.  At Cg < 16 the zero blocks waste 16/Cg of the MFMA work; the
// operation is bandwidth-bound.
//
// MFMA fragment maps (v_mfma_f32_16x16x32_bf16), lane = (r = lane & 15,
// g = lane >> 4):
//   A  lane holds A[row r][k = 8g .. 8g+7]
//   B  lane holds B[k = 8g .. 8g+7][col r]
//   D  lane holds D[row 4g + q][col r], q = 0..3
//
// EXEC rule (docs/KERNELS.md): every MFMA and every transposed LDS read runs
// with EXEC all ones.  No kernel returns early; loop bounds are wave-uniform
// (forward, dgrad: no LDS on the way in) or block-uniform (wgrad); rows past
// the end, taps outside the image and the k tail are ZEROS selected into the
// fragment or stored into the image, never masked lanes.
#include "common.h"

template <int N>
struct GFrag {
  V8 a[N];
};

// ------------------------------------------------------ forward and dgrad --
// One body, two gathers.  Forward: out row m = (n, ho, wo), tap (tr, ts)
// reads x[n][ho·str − pad + tr][wo·str − pad + ts].  Dgrad: out row m =
// (n, hi, wi), tap (tr, ts) reads dz[n][(hi + pad − tr)/str][(wi + pad −
// ts)/str] where both divide; at stride 2 three taps in four are therefore
// zero fragments that still go through the MFMA.  The B element of (k = tap,
// c; column n) is W[n0+n][tap][c'] in forward and W[k0+c][tap][n'] in dgrad,
// primes meaning "within the group"; dgrad reads the weight per element, no
// LDS transpose.
//
//   grid    slabs × m-chunks, flattened, slab fastest (neighbouring blocks
//           read neighbouring 32..64-byte pieces of the same pixels)
//   wave    walks the 16-row tiles w, w+4, .. of the chunk; an A fragment is
//           one 16-byte global load per lane, next tile's loads in flight
//           while this tile's MFMAs run
//   out     bf16 stores, one wave computes an element completely
//   stats   (forward) Σy and Σy² of the unrounded f32 accumulators: a lane
//           keeps column r over all its tiles, the four lane groups meet by
//           xor-shuffle, the four waves in LDS, then one atomic pair per
//           column per block
template <int CS, int R, bool DGRAD>
DEV void gconv_body(const bf16* __restrict__ src, const bf16* __restrict__ w,
                    bf16* __restrict__ dst, float* __restrict__ stats,
                    const GConvP& p, int nslab) {
  constexpr int TAPS = R * R;
  constexpr int NK = TAPS * CS;
  constexpr int NF = (NK + 31) / 32;
  __shared__ float red[4][32];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int slab = blockIdx.x % nslab, chunk = blockIdx.x / nslab;
  const int n0 = slab * 16;
  const int cgs = p.cgs, cgm = p.Cg - 1;
  const int k0 = (n0 >> cgs) << cgs;
  const int C = p.C;
  // output space (OH, OW) and gathered space (SH, SW)
  const int OH = DGRAD ? p.H : p.Ho, OW = DGRAD ? p.W : p.Wo;
  const int SH = DGRAD ? p.Ho : p.H, SW = DGRAD ? p.Wo : p.W;
  const int Mrows = DGRAD ? p.Mi : p.M;
  const int str = p.str, pad = p.pad;

  // ---- B image, once per block ----
  bf16x8 bfrag[NF];
#pragma unroll
  for (int f = 0; f < NF; f++) {
    V8 t;
#pragma unroll
    for (int e = 0; e < 8; e++) {
      const int k = 32 * f + 8 * g + e;
      const int tap = k / CS, kc = k0 + k % CS;
      const int col = n0 + r;
      const bool ok = k < NK && (kc >> cgs) == (col >> cgs);
      const int ko = DGRAD ? kc : col;
      const int cg = (DGRAD ? col : kc) & cgm;
      bf16 v = (bf16)0.f;
      if (ok) v = w[((long)ko * TAPS + tap) * p.Cg + cg];
      t.e[e] = v;
    }
    bfrag[f] = t.v;
  }

  const int mbase = chunk * GCONV_MCHUNK;
  const int ntiles = (min(GCONV_MCHUNK, Mrows - mbase) + 15) >> 4;

  auto load = [&](int t, GFrag<NF>& fr) {
    const int m = mbase + t * 16 + r;
    const bool mok = m < Mrows;
    const int n = m / (OH * OW);
    const int rem = m - n * (OH * OW);
    const int oh = rem / OW, ow = rem - oh * OW;
#pragma unroll
    for (int f = 0; f < NF; f++) {
      const int k = 32 * f + 8 * g;
      const int tap = k / CS, kk = k % CS;
      const int tr = tap / R, ts = tap - tr * R;
      int sh, sw;
      bool ok = mok && tap < TAPS;
      if (DGRAD) {
        const int th = oh + pad - tr, tw = ow + pad - ts;
        ok = ok && th >= 0 && tw >= 0 && ((th | tw) & (str - 1)) == 0;
        sh = th >> (str - 1);
        sw = tw >> (str - 1);
      } else {
        sh = oh * str - pad + tr;
        sw = ow * str - pad + ts;
        ok = ok && sh >= 0 && sw >= 0;
      }
      ok = ok && sh < SH && sw < SW;
      if (ok)
        fr.a[f].u = *(const uint4*)(src + (((long)n * SH + sh) * SW + sw) * C +
                                    k0 + kk);
      else
        fr.a[f].u = uint4{0, 0, 0, 0};
    }
  };

  float s1 = 0.f, s2 = 0.f;
  GFrag<NF> cur, nx;
  if (wave < ntiles) load(wave, cur);
  for (int t = wave; t < ntiles; t += 4) {
    const bool more = t + 4 < ntiles;
    if (more) load(t + 4, nx);
    f32x4 acc = {};
#pragma unroll
    for (int f = 0; f < NF; f++)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur.a[f].v, bfrag[f], acc,
                                                    0, 0, 0);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int row = mbase + t * 16 + 4 * g + q;
      if (row < Mrows) dst[(long)row * C + n0 + r] = f2b(acc[q]);
      if (!DGRAD) {  // rows >= Mrows are exact zeros
        s1 += acc[q];
        s2 += acc[q] * acc[q];
      }
    }
    if (more) cur = nx;
  }

  if (!DGRAD && stats != nullptr) {  // block-uniform
    s1 += __shfl_xor(s1, 16, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (g == 0) {
      red[wave][r] = s1;
      red[wave][16 + r] = s2;
    }
    __syncthreads();
    if (tid < 32) {
      const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      atomicAdd(&stats[tid < 16 ? n0 + tid : C + n0 + tid - 16], v);
    }
  }
}

template <int CS, int R>
__global__ __launch_bounds__(256) void k_gconv_fwd(
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    bf16* __restrict__ y, float* __restrict__ stats, GConvP p, int nslab) {
  gconv_body<CS, R, false>(x, w, y, stats, p, nslab);
}

template <int CS, int R>
__global__ __launch_bounds__(256) void k_gconv_dgrad(
    const bf16* __restrict__ dz, const bf16* __restrict__ w,
    bf16* __restrict__ dx, GConvP p, int nslab) {
  gconv_body<CS, R, true>(dz, w, dx, nullptr, p, nslab);
}

// ------------------------------------------------------------------ wgrad --
// dW[ko][tap][c'] = Σ_m dz[m][ko]·x[pixel(m, tap)][c].  The reduction axis is
// m, so both operands are transposed relative to memory: each 32-row step is
// staged row-major in LDS — dz as [32 m][16 ko], the patch as [32 m][T·CS]
// cut into 64-column images — with 16-byte stores through lds_tr_off<64>,
// and the fragments come back through ds_read_b64_tr_b16 (common.h, the
// scheme of the dense wgrad).  A = dzᵀ (rows ko), B = patch (columns c): the
// accumulator fragment (tap, 16-channel half h) is number tap·CS/16 + h and
// lies at patch column 16·number.
//
//   grid    slabs × msplit, flattened, slab fastest; split s owns rows
//           [s·mchunk, (s+1)·mchunk), mchunk a multiple of 32
//   staging thread (row = tid >> 3, 8 threads per row) loads the row's
//           16-byte runs j = (tid & 7) + 8i, pixel decomposition once per
//           step; threads 0..63 load the dz rows.  The next step's loads are
//           in flight while this step's MFMAs run.
//   waves   split the T·CS/16 accumulator fragments: wave w owns w, w+4, ..
//           (at most 5).  Every wave reads the one dz fragment.  A wave with
//           fewer fragments re-reads its last one and drops the result, so
//           the reads stay block-uniform.  No combine: a wave owns whole dW
//           elements.
//   out     partial == 0: the diagonal blocks are read-add-written into dW;
//           partial != 0: the dense [16][T·CS] tile is stored to the
//           workspace [msplit][slab][16][T·CS] for k_gconv_wgrad_reduce.
DEV bf16x8 gc_read_tr(const bf16* img, int off) {
  const bf16x4 lo = lds_read_tr16(img + off);
  const bf16x4 hi = lds_read_tr16(img + off + 4 * 64);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <int CS, int R>
__global__ __launch_bounds__(256) void k_gconv_wgrad(
    const bf16* __restrict__ x, const bf16* __restrict__ dz,
    float* __restrict__ out, GConvP p, int nslab, int mchunk, int partial) {
  constexpr int TAPS = R * R;
  constexpr int NCOL = TAPS * CS;
  constexpr int NIMG = (NCOL + 63) / 64;  // patch images
  constexpr int NCV = NCOL / 8;           // 16-byte runs of a patch row
  constexpr int NLD = (NCV + 7) / 8;      // runs per staging thread
  constexpr int NFR = NCOL / 16;          // accumulator fragments
  constexpr int NJ = (NFR + 3) / 4;       // per wave
  // image 0: dz (columns 0..15 used); images 1..NIMG: the patch
  __shared__ __attribute__((aligned(16))) bf16 simg[(NIMG + 1) * 2048];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fk = lane >> 4;
  const int slab = blockIdx.x % nslab, split = blockIdx.x / nslab;
  const int ko0 = slab * 16;
  const int cgs = p.cgs;
  const int c0 = (ko0 >> cgs) << cgs;
  const int C = p.C, H = p.H, W = p.W, HoWo = p.Ho * p.Wo, Wo = p.Wo;
  const int str = p.str, pad = p.pad;
  const int mbeg = split * mchunk;
  const int mend = min(p.M, mbeg + mchunk);  // block-uniform

  const int sm = tid >> 3, sc = tid & 7;
  const int dm = tid >> 1, dh = (tid & 1) * 8;  // dz role, tid < 64
  V8 xn[NLD], dn;
  dn.u = uint4{0, 0, 0, 0};
  auto load_tile = [&](int m0) {
    const int m = m0 + sm;
    const bool mok = m < mend;
    const int n = m / HoWo;
    const int rem = m - n * HoWo;
    const int ho = rem / Wo, wo = rem - ho * Wo;
#pragma unroll
    for (int i = 0; i < NLD; i++) {
      const int col = (sc + 8 * i) * 8;
      const int tap = col / CS, c = col % CS;
      const int tr = tap / R, ts = tap - tr * R;
      const int hi = ho * str - pad + tr, wi = wo * str - pad + ts;
      const bool ok = mok && col < NCOL && hi >= 0 && wi >= 0 && hi < H &&
                      wi < W;
      if (ok)
        xn[i].u = *(const uint4*)(x + (((long)n * H + hi) * W + wi) * C + c0 +
                                  c);
      else
        xn[i].u = uint4{0, 0, 0, 0};
    }
    if (tid < 64) {
      if (m0 + dm < mend)
        dn.u = *(const uint4*)(dz + (long)(m0 + dm) * C + ko0 + dh);
      else
        dn.u = uint4{0, 0, 0, 0};
    }
  };

  const int krow = fk * 8 + (fr >> 2);
  const int aoff = lds_tr_off<64>(krow, (fr & 3) * 4);
  int boff[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int col = min(wave + 4 * j, NFR - 1) * 16;
    boff[j] = (1 + (col >> 6)) * 2048 +
              lds_tr_off<64>(krow, (col & 63) + (fr & 3) * 4);
  }

  f32x4 acc[NJ] = {};
  load_tile(mbeg);
  for (int m0 = mbeg; m0 < mend; m0 += 32) {
#pragma unroll
    for (int i = 0; i < NLD; i++) {
      const int col = (sc + 8 * i) * 8;
      if (col < NCOL)
        *(V8*)&simg[(1 + (col >> 6)) * 2048 + lds_tr_off<64>(sm, col & 63)] =
            xn[i];
    }
    if (tid < 64) *(V8*)&simg[lds_tr_off<64>(dm, dh)] = dn;
    __syncthreads();
    if (m0 + 32 < mend) load_tile(m0 + 32);
    const bf16x8 af = gc_read_tr(simg, aoff);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      const bf16x8 bf = gc_read_tr(simg, boff[j]);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[j], 0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int frag = wave + 4 * j;
    if (frag < NFR) {  // wave-uniform; nothing below needs EXEC all ones
      const int tap = frag / (CS / 16), h = frag % (CS / 16);
      const int ca = c0 + h * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = 4 * fk + q, ko = ko0 + row;
        if (partial) {
          out[(((long)split * nslab + slab) * 16 + row) * NCOL + frag * 16 +
              fr] = acc[j][q];
        } else if ((ca >> cgs) == (ko >> cgs)) {
          float* o = out + ((long)ko * TAPS + tap) * p.Cg + (ca & (p.Cg - 1));
          *o = *o + acc[j][q];
        }
      }
    }
  }
}

// Fixed-order sum of the msplit partial tiles into dW (read-add-write), one
// thread per dW element.  ncol = T·CS, ntap = T.
__global__ __launch_bounds__(256) void k_gconv_wgrad_reduce(
    const float* __restrict__ ws, float* __restrict__ dw, long total,
    int msplit, int nslab, int ncol, int ntap, int CS, int Cg, int cgs) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ko = (int)(e / (ntap * Cg));
  const int rem = (int)(e - (long)ko * (ntap * Cg));
  const int tap = rem >> cgs, cg = rem & (Cg - 1);
  const int slab = ko >> 4, row = ko & 15;
  const int c0 = ((slab * 16) >> cgs) << cgs;
  const int ca = ((ko >> cgs) << cgs) + cg;
  const int col = tap * CS + (ca - c0);
  const long pitch = (long)nslab * 16 * ncol;
  const float* s = ws + ((long)slab * 16 + row) * ncol + col;
  float v = s[0];
  for (int i = 1; i < msplit; i++) v += s[i * pitch];
  dw[e] += v;
}

static long g_wgrad_direct = 0, g_wgrad_split = 0;

// -------------------------------------------------------------- launchers --
#define GCONV_DISPATCH(KERNEL, ...)                                        \
  do {                                                                     \
    const int cs_ = p.Cg > 16 ? 32 : 16;                                   \
    if (cs_ == 16 && p.R == 1) KERNEL<16, 1> __VA_ARGS__;                  \
    else if (cs_ == 16) KERNEL<16, 3> __VA_ARGS__;                         \
    else if (p.R == 1) KERNEL<32, 1> __VA_ARGS__;                          \
    else KERNEL<32, 3> __VA_ARGS__;                                        \
  } while (0)

extern "C" {

void launch_gconv_fwd(const void* x, const void* w, void* y, float* stats,
                      GConvP p, hipStream_t st) {
  const int nslab = p.C / 16;
  const int nchunk = (p.M + GCONV_MCHUNK - 1) / GCONV_MCHUNK;
  GCONV_DISPATCH(k_gconv_fwd, <<<nslab * nchunk, 256, 0, st>>>(
      (const bf16*)x, (const bf16*)w, (bf16*)y, stats, p, nslab));
}

void launch_gconv_dgrad(const void* dz, const void* w, void* dx, GConvP p,
                        hipStream_t st) {
  const int nslab = p.C / 16;
  const int nchunk = (p.Mi + GCONV_MCHUNK - 1) / GCONV_MCHUNK;
  GCONV_DISPATCH(k_gconv_dgrad, <<<nslab * nchunk, 256, 0, st>>>(
      (const bf16*)dz, (const bf16*)w, (bf16*)dx, p, nslab));
}

static int gconv_wgrad_mchunk() {
  static const int v = (int)env_long("HZ_GCONV_WGRAD_MCHUNK",
                                     GCONV_WGRAD_MCHUNK);
  return ((v < 32 ? 32 : v) + 31) / 32 * 32;
}

int gconv_wgrad_msplit(GConvP p) {
  const int n = (p.M + gconv_wgrad_mchunk() - 1) / gconv_wgrad_mchunk();
  return n < 1 ? 1 : (n > GCONV_WGRAD_MAXSPLIT ? GCONV_WGRAD_MAXSPLIT : n);
}

long gconv_wgrad_ws_floats(GConvP p, int msplit) {
  const int cs = p.Cg > 16 ? 32 : 16;
  return (long)msplit * p.C * p.R * p.R * cs;
}

void launch_gconv_wgrad(const void* x, const void* dz, float* dw, float* ws,
                        GConvP p, int msplit, hipStream_t st) {
  const int nslab = p.C / 16;
  // rows per split: a multiple of 32 that covers M in msplit pieces
  const int mchunk = ((p.M + msplit - 1) / msplit + 31) / 32 * 32;
  const int partial = msplit > 1;
  GCONV_DISPATCH(k_gconv_wgrad, <<<nslab * msplit, 256, 0, st>>>(
      (const bf16*)x, (const bf16*)dz, partial ? ws : dw, p, nslab, mchunk,
      partial));
  if (partial) {
    const int cs = p.Cg > 16 ? 32 : 16;
    const long total = (long)p.C * p.R * p.R * p.Cg;
    k_gconv_wgrad_reduce<<<(int)((total + 255) / 256), 256, 0, st>>>(
        ws, dw, total, msplit, nslab, p.R * p.R * cs, p.R * p.R, cs, p.Cg,
        p.cgs);
    g_wgrad_split++;
  } else {
    g_wgrad_direct++;
  }
}

void gconv_wgrad_launch_counts(long* direct, long* split) {
  *direct = g_wgrad_direct;
  *split = g_wgrad_split;
}

}  // extern "C"
