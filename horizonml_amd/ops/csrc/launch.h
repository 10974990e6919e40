// The host/kernel boundary of the horizonml_amd kernel set, defined once.
//
// Everything that crosses between bind.cpp (g++) and the *.hip translation
// units (hipcc) lives here: the structs that travel as kernel arguments,
// the magic-division generator that fills them, the extern "C" launcher
// declarations, and the environment-knob reader.  Both sides include this
// header, so a launcher whose definition drifts from its declaration, or a
// struct field added on one side only, is a compile error instead of a
// kernel reading garbage.  Plain C++17: no device code, no torch.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdlib>
#include <type_traits>

// ------------------------------------------------------------- ABI structs --
struct ConvP {
  int Nb, H, W, C, K;      // batch, input spatial, in/out channels
  int Ho, Wo, R, S;        // output spatial, filter
  int str, pad;
  int M, Kd;               // GEMM rows, reduction size
  // Tap window (clip_taps below).  R, S, Kd describe the window the kernels
  // loop over; the filter in memory is Rf×Sf and the window starts at tap
  // (r0, s0).  Unclipped: r0 = s0 = 0, Rf = R, Sf = S.
  int r0, s0, Rf, Sf;
};

// Fast division by a runtime constant (cutlass FastDivmod form):
// q = (umulhi(n, m) + n) >> s for 1 < d < 2^31, 0 <= n < 2^31; d == 1 is
// the identity.  The implicit-GEMM gathers decompose linear indices with
// 4-5 divisions per vec8 — emulated u32 division costs ~25-40 VALU each.
struct MagicP {
  unsigned m[4];
  int s[4];
  unsigned d[4];
};

// Batched (deferred) wgrad task tables.  X/Dz are bf16 tensors; the kernel
// casts them where it calls wgrad_tile.
constexpr int WG_MAX_TASKS = 20;

struct WgradTask {
  const void* X;
  const void* Dz;
  float* out;      // dW when msplit==1, else slab base [msplit][Ntot][Kd]
  ConvP p;
  MagicP mg;
  int Ntot, mchunk, msplit, tx, ty;  // tile counts
  int base;        // first block id of this task
  int vec;
};

struct WgradBatchArgs {
  int n;
  WgradTask t[WG_MAX_TASKS];
};

struct WredTask {
  const float* ws;
  float* dW;
  long n;
  int msplit;
  int base;  // first block id; each block covers 1024 floats
  // Clipped task (Kd > 0): the slabs are dense [K][Kd] over the tap window
  // and dW is the full filter.  Slab element (ko, k3) lands at
  //   ko*KdF + org + k3 + (k3 / SC)*skip
  // with SC = S*C, KdF = Rf*Sf*C, org = (r0*Sf + s0)*C, skip = (Sf - S)*C.
  // Kd == 0: dW index = slab index.
  int Kd, SC, KdF, org, skip;
};

// Fills the scatter fields of a slab-reduce task from the conv's geometry.
inline void wred_set_window(WredTask* t, const ConvP& p) {
  const bool clipped = p.R != p.Rf || p.S != p.Sf;
  t->Kd = clipped ? p.Kd : 0;
  t->SC = p.S * p.C;
  t->KdF = p.Rf * p.Sf * p.C;
  t->org = (p.r0 * p.Sf + p.s0) * p.C;
  t->skip = (p.Sf - p.S) * p.C;
}

struct WredBatchArgs {
  int n;
  WredTask t[WG_MAX_TASKS];
};

// Both batch-argument structs travel as kernel arguments BY VALUE (no
// staging buffers, hipGraph-capture-safe), so they must be plain bytes and
// fit the 4 KB kernarg segment.
static_assert(sizeof(WgradBatchArgs) <= 4096 && sizeof(WredBatchArgs) <= 4096,
              "batched wgrad task tables must fit the kernarg segment");
static_assert(std::is_trivially_copyable_v<WgradBatchArgs> &&
                  std::is_trivially_copyable_v<WredBatchArgs>,
              "batched wgrad task tables are copied into the kernarg segment");

// Weight layout handed to launch_conv_dgrad.
enum DgradWLayout { DGRAD_W_RSCK = 0, DGRAD_W_KRSC = 1 };

// ---------------------------------------------------------- magic division --
inline void magic_u32(unsigned d, unsigned* m, int* sh) {
  if (d <= 1) { *m = 0; *sh = 0; return; }
  int p = 0;
  while ((1ull << p) < d) p++;
  *m = (unsigned)((((unsigned long long)((1ull << p) - d) << 32) / d) + 1);
  *sh = p;
}

// gather divisors per mode: MODE1 {Ho*Wo, Wo, S*C, C};
// MODE2 {H*W, W, S*K, K} (index 3 also serves b_addr's /K %K)
inline MagicP make_magic(const ConvP& p, int mode) {
  MagicP mg{};
  unsigned d[4];
  if (mode == 2) {
    d[0] = (unsigned)(p.H * p.W);
    d[1] = (unsigned)p.W;
    d[2] = (unsigned)(p.S * p.K);
    d[3] = (unsigned)p.K;
  } else {
    d[0] = (unsigned)(p.Ho * p.Wo);
    d[1] = (unsigned)p.Wo;
    d[2] = (unsigned)(p.S * p.C);
    d[3] = (unsigned)p.C;
  }
  for (int i = 0; i < 4; i++) {
    mg.d[i] = d[i] ? d[i] : 1;
    magic_u32(mg.d[i], &mg.m[i], &mg.s[i]);
  }
  return mg;
}

// -------------------------------------------------------------- tap window --
// Filter taps that only ever meet padding: tap row r is live iff some output
// row ho in [0, Ho) reads a real input row, 0 <= ho*str - pad + r < H.
// Returns the bounding range [*lo, *lo + *n) of the live taps of one axis
// (a dead tap inside the range stays and multiplies zeros); n == 0 when no
// tap is live.
inline void tap_range(int H, int Ho, int R, int str, int pad, int* lo,
                      int* n) {
  int first = R, last = -1;
  for (int r = 0; r < R; r++)
    for (int ho = 0; ho < Ho; ho++) {
      const int hi = ho * str - pad + r;
      if (hi >= 0 && hi < H) {
        if (r < first) first = r;
        last = r;
        break;
      }
    }
  *lo = last < 0 ? 0 : first;
  *n = last < 0 ? 0 : last - first + 1;
}

// Clips a full-filter ConvP (Rf = R, Sf = S, r0 = s0 = 0) to its tap window:
// R, S, Kd become the window's and (r0, s0) its origin in the Rf×Sf filter.
// The (input pixel, output pixel, tap) relation is the same in forward,
// dgrad and wgrad, so one window serves all three.  Ho, Wo, M keep the full
// filter's values.  A conv with no live tap on an axis is left unclipped.
inline ConvP clip_taps(ConvP p) {
  int r0, rn, s0, sn;
  tap_range(p.H, p.Ho, p.Rf, p.str, p.pad, &r0, &rn);
  tap_range(p.W, p.Wo, p.Sf, p.str, p.pad, &s0, &sn);
  if (rn <= 0 || sn <= 0) return p;
  p.r0 = r0;
  p.s0 = s0;
  p.R = rn;
  p.S = sn;
  p.Kd = rn * sn * p.C;
  return p;
}

inline bool taps_clipped(const ConvP& p) {
  return p.R != p.Rf || p.S != p.Sf;
}

// The tap window of a conv's geometry whether or not `p` was clipped: what
// the window registry (bind.cpp) records.  A tap outside it has an exactly
// zero weight gradient with clipping off too.
inline ConvP geometric_taps(ConvP p) {
  p.r0 = p.s0 = 0;
  p.R = p.Rf;
  p.S = p.Sf;
  p.Kd = p.Rf * p.Sf * p.C;
  return clip_taps(p);
}

// ------------------------------------------------------- environment knobs --
// Every HZ_* knob is read once, as
//   static const T x = (T)env_long("HZ_...", dflt);
// at its point of use (docs/TUNING.md lists them all).
inline long env_long(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}

// --------------------------------------------------------------- launchers --
// Activation tensors are bf16 NHWC behind void*; statistics, parameters and
// workspaces are f32.
extern "C" {

// conv_kernels.hip
int conv_fwd_splitk(ConvP p);
int conv_dgrad_splitk(ConvP p);
void launch_conv_fwd(const void* x, const void* w, void* y, float* stats,
                     ConvP p, hipStream_t st);
void launch_conv_fwd_splitk(const void* x, const void* w, float* ws, ConvP p,
                            int splitk, hipStream_t st);
// w_layout says what `w` is: the RSCK image, or the KRSC weight itself
void launch_conv_dgrad(const void* dz, const void* w, void* dx, float* ws,
                       int splitk, ConvP p, int accum, int w_layout,
                       hipStream_t st);
void launch_gemm_bf16(const void* a, const void* b, void* c, int M, int N,
                      int K, hipStream_t st);
int wgrad_msplit(ConvP p);
// tr != 0: row-major LDS images with transposed reads; 0: transposed scatter
void launch_wgrad(const void* x, const void* dz, float* dw, float* ws,
                  ConvP p, int tr, hipStream_t st);
void launch_wgrad_batched_t(const WgradBatchArgs* args, int blocks, int tk3,
                            int tko, int tr, hipStream_t st);
void launch_wgrad_reduce_batched(const WredBatchArgs* args, int blocks,
                                 hipStream_t st);

// elem_kernels.hip: switches and queries
void set_kernels_deterministic(int on);
void set_kernels_bn_owner(int on);
int kernels_bn_owner();
void bn_owner_launch_counts(long* fwd, long* bwd);
int bn_owner_fwd_pick(long M, int C, int lpr_req);
int bn_owner_bwd_pick(long M, int C, int lpr_req);

// elem_kernels.hip: BatchNorm
void launch_bn_apply(const void* x, const void* res, void* y,
                     const float* stats, const float* gamma,
                     const float* beta, float* rmean, float* rvar,
                     float* smean, float* sinvstd, long M, int C,
                     float momentum, float eps, int training, int act,
                     hipStream_t st);
void launch_bn_apply_f32(const float* ws, const void* res, void* y,
                         void* convout, const float* stats,
                         const float* gamma, const float* beta, float* rmean,
                         float* rvar, float* smean, float* sinvstd, long M,
                         int C, float momentum, float eps, int training,
                         int act, int nsplit, hipStream_t st);
void launch_stats_reduce(const float* ws, float* stats, long M, int C,
                         int nsplit, hipStream_t st);
void launch_stats_bf16_det(const void* x, float* stats, long M, int C,
                           hipStream_t st);
void launch_cast_f32_bf16(const float* src, void* dst, long n, int nsplit,
                          int accum, hipStream_t st);
void launch_cast_bnact(const float* src, void* dst, long M, int C, int nsplit,
                       int accum, const void* x_up, const void* y_up,
                       const float* smean, const float* sinvstd,
                       const float* gamma, const float* beta, float* sum_dz,
                       float* sum_dzx, int mask_mode, hipStream_t st);
void launch_bnact_bwd_reduce(const void* dy, const void* yout, const void* x,
                             const float* smean, const float* sinvstd,
                             const float* gamma, const float* beta,
                             float* sum_dz, float* sum_dzx, long M, int C,
                             int mask_mode, hipStream_t st);
void launch_bn_bwd_apply(const void* dy, const void* yout, const void* x,
                         const float* smean, const float* sinvstd,
                         const float* gamma, const float* beta,
                         const float* sum_dz, const float* sum_dzx,
                         void* dconv, void* dres, long M, int C,
                         int mask_mode, hipStream_t st);
void launch_bn_fwd_owner(const float* ws, const void* res, void* y,
                         void* convout, const float* gamma,
                         const float* beta, float* rmean, float* rvar,
                         float* smean, float* sinvstd, long M, int C,
                         float momentum, float eps, int act, int nsplit,
                         int lpr, hipStream_t st);
void launch_bn_bwd_owner(const void* dy, const void* yout, const void* x,
                         const float* smean, const float* sinvstd,
                         const float* gamma, const float* beta,
                         float* sum_dz, float* sum_dzx, void* dconv,
                         void* dres, long M, int C, int mask_mode, int lpr,
                         hipStream_t st);

// elem_kernels.hip: depthwise conv, pools, classifier, loss
void launch_dw_fwd(const void* x, const void* w, void* y, float* stats,
                   int Nb, int H, int W, int C, int Ho, int Wo, int R, int S,
                   int str, int pad, hipStream_t st);
void launch_dw_dgrad(const void* dz, const void* w, void* dx, int Nb, int H,
                     int W, int C, int Ho, int Wo, int R, int S, int str,
                     int pad, hipStream_t st);
void launch_dw_wgrad(const void* x, const void* dz, float* dw, int Nb, int H,
                     int W, int C, int Ho, int Wo, int R, int S, int str,
                     int pad, hipStream_t st);
void launch_maxpool_fwd(const void* x, void* y, unsigned char* idx, int Nb,
                        int H, int W, int C, int Hp, int Wp, hipStream_t st);
void launch_maxpool_bwd(const void* dy, const unsigned char* idx, void* dx,
                        int Nb, int H, int W, int C, int Hp, int Wp,
                        hipStream_t st);
void launch_avgpool_fwd(const void* x, void* y, int Nb, int HW, int C,
                        hipStream_t st);
void launch_avgpool_bwd(const void* dy, void* dx, int Nb, int HW, int C,
                        hipStream_t st);
void launch_linear_fwd(const void* x, const void* w, const float* b, float* y,
                       int B, int In, int Out, hipStream_t st);
void launch_linear_bwd(const float* dy, const void* x, const void* w,
                       void* dx, float* dw, float* db, int B, int In, int Out,
                       int accum, hipStream_t st);
void launch_ce_fwd_bwd(const float* logits, const long* target, float* loss,
                       float* dlogits, int B, int NC, hipStream_t st);
void launch_ce_ls_fwd_bwd(const float* logits, const long* target,
                          float* loss, float* dlogits, int B, int NC,
                          float eps, hipStream_t st);

// elem_kernels.hip: optimizers.  step_t is the device step counter; the
// Adam launchers (and SGD with a table) increment it before the update.
void launch_adam_step(float* master, float* grad, float* m, float* v,
                      void* shadow, float* step_t, long n, float lr, float b1,
                      float b2, float eps, float wd, int zero_grad,
                      float* extra_zero, long n_extra, const void* gsrc,
                      float gscale, float* prev, float* sumsq, float* divout,
                      hipStream_t st);
void launch_sgd_step(float* master, float* grad, float* mom, void* shadow,
                     long n, float lr, float mu, float wd, int zero_grad,
                     const void* gsrc, float gscale, float* prev,
                     float* sumsq, float* divout, hipStream_t st);
void launch_adam_step_ex(float* master, float* grad, float* m, float* v,
                         void* shadow, float* step_t, long n, float lr,
                         float b1, float b2, float eps, float wd,
                         int zero_grad, float* extra_zero, long n_extra,
                         const void* gsrc, float gscale, float* prev,
                         float* sumsq, float* divout, const float* lr_table,
                         long T, float* lr_out, int decoupled,
                         hipStream_t st);
void launch_sgd_step_ex(float* master, float* grad, float* mom, void* shadow,
                        long n, float lr, float mu, float wd, int zero_grad,
                        const void* gsrc, float gscale, float* prev,
                        float* sumsq, float* divout, float* step_t,
                        const float* lr_table, long T, float* lr_out,
                        int nesterov, hipStream_t st);
// Segmented forms: chunks int32 [nchunks][3] = (segment, start, length),
// seg_meta int32 [nseg][3] = (chunk begin, chunk end, flags), seg_mul f32
// [nseg][2] = (gmul, wmul).  launch_seg_norms is the two-dispatch norm
// reduction (partials, finalize) that fills seg_mul and norm_out = (N, c).
void launch_seg_norms(const float* master, const float* grad,
                      const void* gsrc, float gscale, const int* chunks,
                      int nchunks, const int* seg_meta, int nseg,
                      float* partials, float* seg_norms, float* seg_mul,
                      float* norm_out, float wd, float max_norm, int lars,
                      float eta, hipStream_t st);
void launch_adam_step_seg(float* master, float* grad, float* m, float* v,
                          void* shadow, float* step_t, float lr, float b1,
                          float b2, float eps, int zero_grad,
                          float* extra_zero, long n_extra, const void* gsrc,
                          float gscale, float* prev, float* sumsq,
                          float* divout, const float* lr_table, long T,
                          float* lr_out, int decoupled, const int* chunks,
                          int nchunks, const float* seg_mul, hipStream_t st);
void launch_sgd_step_seg(float* master, float* grad, float* mom, void* shadow,
                         float lr, float mu, int zero_grad, const void* gsrc,
                         float gscale, float* prev, float* sumsq,
                         float* divout, float* step_t, const float* lr_table,
                         long T, float* lr_out, int nesterov,
                         const int* chunks, int nchunks, const float* seg_mul,
                         hipStream_t st);
// Live-range forms (no weight decay): live int32 [nchunks][4] = (start,
// run_len, run_pitch, nruns), 16-byte aligned; one workgroup per chunk
// updates elements start + r*run_pitch + j, r < nruns, j < run_len, and
// nothing else of the flat buffers.
void launch_adam_step_live(float* master, float* grad, float* m, float* v,
                           void* shadow, float* step_t, float lr, float b1,
                           float b2, float eps, int zero_grad,
                           float* extra_zero, long n_extra, const void* gsrc,
                           float gscale, float* prev, float* sumsq,
                           float* divout, const float* lr_table, long T,
                           float* lr_out, const int* live, int nchunks,
                           hipStream_t st);
void launch_sgd_step_live(float* master, float* grad, float* mom,
                          void* shadow, float lr, float mu, int zero_grad,
                          const void* gsrc, float gscale, float* prev,
                          float* sumsq, float* divout, float* step_t,
                          const float* lr_table, long T, float* lr_out,
                          int nesterov, const int* live, int nchunks,
                          hipStream_t st);

// elem_kernels.hip: layout, probes, input pipeline
void launch_permute_krsc_rsck(const void* src, void* dst, const int* meta,
                              int nconv, int max_elem, hipStream_t st);
void launch_grad_divergence(const float* g, float* prev, float* sumsq,
                            float* out, long n, int skip_first,
                            hipStream_t st);
void launch_normalize_u8(const void* x, void* y, long total, int C, long HW,
                         float mean, float std, hipStream_t st);
void launch_augment_normalize_u8(const void* x, void* y, void* state,
                                 const int* params, long N, int C, int H,
                                 int W, int pad, int flip, float mean,
                                 float std, hipStream_t st);

}  // extern "C"
