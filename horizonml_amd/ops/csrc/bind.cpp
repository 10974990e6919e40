// Torch bindings for the horizonml_amd gfx950 kernel set.
// Compiled host-side (g++); all device code lives in *.hip translation units
// linked as extra objects (no hipify, no CUDA compat).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPCachingAllocator.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "launch.h"  // ABI structs, launcher declarations, env_long

namespace {

using torch::Tensor;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// Deterministic mode: fixed-order reductions replace every atomic-order
// dependence (BN batch stats, backward channel sums, CE loss scalar).
// Measured: bitwise run-to-run reproducible at ~9x step time (bs=64) —
// the single-block serial reductions dominate at small batches; a
// reproducibility/debugging tool.  Weight gradients are already
// deterministic (atomic-free slab reduction in a fixed z order).
bool g_deterministic = false;
void set_deterministic(bool on) {
  g_deterministic = on;
  set_kernels_deterministic(on ? 1 : 0);
}
bool deterministic_enabled() { return g_deterministic; }

// Channel-owner BatchNorm (single-launch reduce+apply at small M): runtime
// switch so one process can run both dispatches (tests, A/B timing).
// Deterministic mode always keeps the two-kernel dispatch.
void set_bn_owner(bool on) { set_kernels_bn_owner(on ? 1 : 0); }
bool bn_owner_enabled() { return kernels_bn_owner() != 0; }
// (forward, backward) owner-kernel launches so far in this process.
std::vector<int64_t> bn_owner_launches() {
  long f = 0, b = 0;
  bn_owner_launch_counts(&f, &b);
  return {(int64_t)f, (int64_t)b};
}

// KRSC-direct dgrad: dgrad reads the KRSC weights themselves, so no RSCK
// image is kept or rebuilt per step.  The switch (HZ_DGRAD_KRSC, read at
// load, default on) is what the Python side consults when it decides whether
// to build an RSCK image and pass it in conv_bn_act_bwd's w_rsck slot; the
// slot, not the switch, selects the kernel (dgrad_dx).  Off = the former
// RSCK path, kept for A/B timing.
bool g_dgrad_krsc = env_long("HZ_DGRAD_KRSC", 1) != 0;
void set_dgrad_krsc(bool on) { g_dgrad_krsc = on; }
bool dgrad_krsc_enabled() { return g_dgrad_krsc; }

// Wgrad m-loop body (conv_kernels.hip, "Row-major form").  HZ_WGRAD_TR (read
// at load, default on) selects row-major LDS images with transposed fragment
// reads; off = the former transposed 2-byte scatter, bitwise the same dW,
// kept for A/B timing and as the tests' reference.
bool g_wgrad_tr = env_long("HZ_WGRAD_TR", 1) != 0;
void set_wgrad_tr(bool on) { g_wgrad_tr = on; }
bool wgrad_tr_enabled() { return g_wgrad_tr; }

// Tap window (launch.h, clip_taps): forward, dgrad and wgrad skip the filter
// taps that only ever meet padding.  HZ_TAP_CLIP (read at load, default on);
// off = every conv walks its whole filter, kept for A/B timing and as the
// tests' reference.  Consulted in one place, make_convp.
bool g_tap_clip = env_long("HZ_TAP_CLIP", 1) != 0;
void set_tap_clip(bool on) { g_tap_clip = on; }
bool tap_clip_enabled() { return g_tap_clip; }

// (r0, s0, R', S') of a conv's tap window, whatever the switch says.
std::vector<int64_t> conv_tap_window(int64_t H, int64_t W, int64_t R,
                                     int64_t S, int64_t stride, int64_t pad) {
  TORCH_CHECK(stride >= 1 && pad >= 0 && R >= 1 && S >= 1 &&
                  H + 2 * pad >= R && W + 2 * pad >= S,
              "conv_tap_window: empty output or bad geometry");
  ConvP p{};
  p.H = (int)H;
  p.W = (int)W;
  p.C = 1;
  p.R = p.Rf = (int)R;
  p.S = p.Sf = (int)S;
  p.str = (int)stride;
  p.pad = (int)pad;
  p.Ho = (p.H + 2 * p.pad - p.R) / p.str + 1;
  p.Wo = (p.W + 2 * p.pad - p.S) / p.str + 1;
  p = clip_taps(p);
  return {p.r0, p.s0, p.R, p.S};
}

// ---- tap-window registry ----------------------------------------------------
// What the fused optimizer needs to skip dead filter taps (engine/flat.py,
// live table): per weight-gradient buffer, the filter shape and the union of
// the tap windows of every geometry its conv has run a direct-grad backward
// at.  Host bookkeeping only: nothing is launched or allocated on the device,
// so it runs the same under graph capture.  Monotone: a window only widens;
// the version counts creations and growths.
struct TapWindow {
  int K, Rf, Sf, C;
  int r0, R, s0, S;
};
std::mutex g_tapwin_mu;  // backward runs on autograd's device thread
std::unordered_map<uintptr_t, TapWindow> g_tapwin;
int64_t g_tapwin_version = 0;

void record_tap_window(const Tensor& dw, const ConvP& p) {
  const ConvP g = geometric_taps(p);
  const uintptr_t key = (uintptr_t)dw.data_ptr();
  std::lock_guard<std::mutex> lock(g_tapwin_mu);
  auto it = g_tapwin.find(key);
  if (it == g_tapwin.end() || it->second.K != g.K || it->second.Rf != g.Rf ||
      it->second.Sf != g.Sf || it->second.C != g.C) {
    // new buffer, or its address now belongs to another filter
    g_tapwin[key] = {g.K, g.Rf, g.Sf, g.C, g.r0, g.R, g.s0, g.S};
    g_tapwin_version++;
    return;
  }
  TapWindow& w = it->second;
  const int r0 = std::min(w.r0, g.r0), s0 = std::min(w.s0, g.s0);
  const int r1 = std::max(w.r0 + w.R, g.r0 + g.R);
  const int s1 = std::max(w.s0 + w.S, g.s0 + g.S);
  if (r0 != w.r0 || s0 != w.s0 || r1 - r0 != w.R || s1 - s0 != w.S) {
    w.r0 = r0;
    w.R = r1 - r0;
    w.s0 = s0;
    w.S = s1 - s0;
    g_tapwin_version++;
  }
}

// [(grad data pointer, K, Rf, Sf, C, r0, R, s0, S)], in no particular order
std::vector<std::vector<int64_t>> tap_window_registry() {
  std::lock_guard<std::mutex> lock(g_tapwin_mu);
  std::vector<std::vector<int64_t>> out;
  out.reserve(g_tapwin.size());
  for (const auto& kv : g_tapwin) {
    const TapWindow& w = kv.second;
    out.push_back({(int64_t)kv.first, w.K, w.Rf, w.Sf, w.C, w.r0, w.R, w.s0,
                   w.S});
  }
  return out;
}

int64_t tap_window_version() {
  std::lock_guard<std::mutex> lock(g_tapwin_mu);
  return g_tapwin_version;
}

// Forget the windows of the buffers at addresses [lo, hi); every window when
// hi <= lo.  A manager calls it over its freshly allocated gradient buffer,
// whose addresses may have served another model's filters before.  The
// version still moves forward, so a table built from the old entries reads
// as stale.
void tap_window_reset(int64_t lo, int64_t hi) {
  std::lock_guard<std::mutex> lock(g_tapwin_mu);
  if (hi <= lo) {
    g_tapwin.clear();
  } else {
    for (auto it = g_tapwin.begin(); it != g_tapwin.end();)
      if (it->first >= (uintptr_t)lo && it->first < (uintptr_t)hi)
        it = g_tapwin.erase(it);
      else
        ++it;
  }
  g_tapwin_version++;
}

// Live-range optimizer step (engine/flat.py): HZ_OPT_SKIP_DEAD (read at
// load, default on); off = the optimizers launch the full-range kernels,
// kept for A/B timing and as the tests' reference.
bool g_opt_skip_dead = env_long("HZ_OPT_SKIP_DEAD", 1) != 0;
void set_opt_skip_dead(bool on) { g_opt_skip_dead = on; }
bool opt_skip_dead_enabled() { return g_opt_skip_dead; }

// ---- deferred (batched) wgrad ---------------------------------------------
// The weight-gradient GEMMs are off the backward's critical chain (nothing
// reads dW until the optimizer step), and each conv's own wgrad underfills
// the 256 CUs at CIFAR shapes.  In direct-grad mode with defer enabled
// (FlatParamManager), conv backward only records the task; ``flush_wgrad``
// (called by the fused optimizer / before the DP all-reduce) then runs ALL
// pending weight gradients as one batched kernel + one batched slab-reduce —
// 2 launches instead of ~40, full chip occupancy, no atomics.  Task tables
// travel as kernel arguments by value, so the path is hipGraph-capture-safe
// (no host staging buffers whose contents could change between replays).
struct PendingWgrad {
  torch::Tensor x, dconv, dw;
  ConvP p;
};

bool g_wgrad_defer = false;
std::vector<PendingWgrad> g_pending;
torch::Tensor g_wgrad_ws;  // persistent slab workspace (grows on demand)

void set_wgrad_defer(bool on) { g_wgrad_defer = on; }
bool wgrad_defer_enabled() { return g_wgrad_defer; }
int64_t wgrad_pending() { return (int64_t)g_pending.size(); }

static inline int cdiv_i(long a, long b) { return (int)((a + b - 1) / b); }

void flush_one_group(int lo, int hi);

// Tasks writing the SAME grad tensor (gradient accumulation: several
// backwards before one flush) must not RMW concurrently — partition the
// pending list into maximal runs of unique dW targets and flush each run
// as its own batched launch pair (runs are stream-ordered).
void flush_wgrad() {
  if (g_pending.empty()) return;
  const int total = (int)g_pending.size();
  int lo = 0;
  while (lo < total) {
    std::vector<const void*> seen;
    int hi = lo;
    for (; hi < total; hi++) {
      const void* ptr = g_pending[hi].dw.data_ptr();
      bool dup = false;
      for (const void* q : seen)
        if (q == ptr) { dup = true; break; }
      if (dup) break;
      seen.push_back(ptr);
    }
    flush_one_group(lo, hi);
    lo = hi;
  }
  g_pending.clear();
}

// Flush only the pending wgrads whose dW target lies inside the flat
// gradient range [lo_elem, hi_elem) of `flat` (the FlatParamManager grad
// buffer) — the per-bucket flush of the overlapped DP all-reduce
// (parallel/flat_reducer.py).  Entries outside the range stay pending for
// their own bucket.  Reuses flush_wgrad's dup-partitioned batched launch
// by swapping the matching run into g_pending.
void flush_wgrad_range(torch::Tensor flat, int64_t lo_elem, int64_t hi_elem) {
  if (g_pending.empty()) return;
  const char* base = (const char*)flat.data_ptr();
  const char* plo = base + lo_elem * flat.element_size();
  const char* phi = base + hi_elem * flat.element_size();
  std::vector<PendingWgrad> take, keep;
  for (auto& p : g_pending) {
    const char* q = (const char*)p.dw.data_ptr();
    if (q >= plo && q < phi)
      take.push_back(std::move(p));
    else
      keep.push_back(std::move(p));
  }
  g_pending = std::move(take);
  flush_wgrad();  // clears g_pending
  g_pending = std::move(keep);
}

void flush_one_group(int group_lo, int group_hi) {
  auto st = cur_stream();
  const int n = group_hi - group_lo;
  const PendingWgrad* pend = g_pending.data() + group_lo;
  // split choice: mchunk ≈ 512 rows keeps per-block m-loops short while the
  // batched grid (all tasks together) fills the chip
  std::vector<int> msplit(n), mchunk(n);
  std::vector<long> ws_off(n, 0);
  long ws_total = 0;
  for (int i = 0; i < n; i++) {
    const ConvP& p = pend[i].p;
    // large-M tasks take 2048-row chunks: the batched grid pools every
    // task's blocks so per-task fill matters less than slab volume — at
    // mchunk 512 a ResNet50 layer1 conv makes 196 f32 slabs whose
    // write+reduce traffic dominated wgrad_reduce (r02 traces)
    static const int mc_small = (int)env_long("HZ_WG_MCHUNK", 512);
    const int mc_base = p.M >= 32768 ? 2048 : mc_small;
    int ms = std::max(1, cdiv_i(p.M, mc_base));
    int mc = cdiv_i(cdiv_i(p.M, ms), 32) * 32;
    ms = cdiv_i(p.M, mc);
    msplit[i] = ms;
    mchunk[i] = mc;
    if (ms > 1) {
      ws_off[i] = ws_total;
      ws_total += (long)ms * p.K * p.Kd;
    }
  }
  if (ws_total > 0 &&
      (!g_wgrad_ws.defined() || g_wgrad_ws.numel() < ws_total))
    g_wgrad_ws = at::empty({ws_total},
                           pend[0].x.options().dtype(torch::kFloat32));
  float* ws_base = ws_total > 0 ? g_wgrad_ws.data_ptr<float>() : nullptr;

  // four tile classes (tk3, tko ∈ {64,128}): 128-wide k3 for big-Kd
  // large-M tasks halves the Dz re-read; 128-wide ko for K>=128 tasks
  // halves the X re-read — separate launches keep per-class LDS/occupancy
  auto tk3_of = [](const ConvP& p) {
    // swept on MI355X (r50 224 + bs1024)
    static const int kd_min = (int)env_long("HZ_WG_TK3_KD", 256);
    // swept on MI355X: M=2048 admits CIFAR-bs64 layer1 (M=4096) and
    // costs ~2% at the parity point; 5000 keeps r50@224 at 9.39 ms
    static const int m_min = (int)env_long("HZ_WG_TK3_M", 5000);
    // a clipped task (tap window) stays in the 64-wide classes, the only
    // ones whose kernels carry the window form of wgrad_tile
    if (taps_clipped(p)) return 64;
    return (p.Kd >= kd_min && p.M >= m_min) ? 128 : 64;
  };
  auto tko_of = [](const ConvP& p) {
    static const int k_min = (int)env_long("HZ_WG_TKO_K", 128);
    return p.K >= k_min ? 128 : 64;
  };
  for (int cls = 0; cls < 4; cls++) {
    const int tk3 = (cls & 1) ? 128 : 64;
    const int tko = (cls & 2) ? 128 : 64;
    std::vector<int> idx;
    for (int i = 0; i < n; i++)
      if (tk3_of(pend[i].p) == tk3 && tko_of(pend[i].p) == tko)
        idx.push_back(i);
    for (size_t lo = 0; lo < idx.size(); lo += WG_MAX_TASKS) {
      WgradBatchArgs a{};
      a.n = (int)std::min((size_t)WG_MAX_TASKS, idx.size() - lo);
      int blocks = 0;
      for (int j = 0; j < a.n; j++) {
        const int i = idx[lo + j];
        const PendingWgrad& pw = pend[i];
        WgradTask& t = a.t[j];
        t.X = pw.x.data_ptr();
        t.Dz = pw.dconv.data_ptr();
        t.out = msplit[i] > 1 ? ws_base + ws_off[i]
                              : pw.dw.data_ptr<float>();
        t.p = pw.p;
        t.mg = make_magic(pw.p, 1);
        t.Ntot = pw.p.K;
        t.mchunk = mchunk[i];
        t.msplit = msplit[i];
        t.tx = cdiv_i(pw.p.Kd, tk3);
        t.ty = cdiv_i(pw.p.K, tko);
        t.base = blocks;
        t.vec = (pw.p.C % 8) == 0;
        blocks += t.tx * t.ty * t.msplit;
      }
      launch_wgrad_batched_t(&a, blocks, tk3, tko, (int)g_wgrad_tr, st);
    }
  }

  // batched slab reduce for the split tasks
  WredBatchArgs r{};
  r.n = 0;
  int rblocks = 0;
  auto flush_red = [&]() {
    if (r.n > 0) launch_wgrad_reduce_batched(&r, rblocks, st);
    r.n = 0;
    rblocks = 0;
  };
  for (int i = 0; i < n; i++) {
    if (msplit[i] <= 1) continue;
    if (r.n == WG_MAX_TASKS) flush_red();
    WredTask& t = r.t[r.n++];
    t.ws = ws_base + ws_off[i];
    t.dW = pend[i].dw.data_ptr<float>();
    t.n = (long)pend[i].p.K * pend[i].p.Kd;
    wred_set_window(&t, pend[i].p);
    t.msplit = msplit[i];
    t.base = rblocks;
    rblocks += cdiv_i(t.n, 1024);
  }
  flush_red();
}

void check_cl(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4, name, " must be 4-D");
  bool cl = t.is_contiguous(at::MemoryFormat::ChannelsLast);
  bool hw1 = t.size(2) == 1 && t.size(3) == 1 && t.is_contiguous();
  TORCH_CHECK(cl || hw1, name, " must be channels_last contiguous");
}

void check_f32(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.is_contiguous(),
              name, " must be contiguous f32 on GPU");
}

// data pointer of an optional tensor, nullptr when absent
template <class T>
T* opt_ptr(const c10::optional<Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}
void* opt_ptr(const c10::optional<Tensor>& t) {
  return t.has_value() ? t->data_ptr() : nullptr;
}

void check_probe(const c10::optional<Tensor>& prev,
                 const c10::optional<Tensor>& sumsq,
                 const c10::optional<Tensor>& out) {
  TORCH_CHECK(prev.has_value() == sumsq.has_value()
                  && prev.has_value() == out.has_value(),
              "probe tensors must be passed together");
}

Tensor empty_cl_bf16(int64_t n, int64_t c, int64_t h, int64_t w,
                     const Tensor& like) {
  return at::empty({n, c, h, w},
                   like.options().dtype(torch::kBFloat16),
                   at::MemoryFormat::ChannelsLast);
}

// Forward geometry of one conv, clipped to its tap window when the switch is
// on: the one place every conv entry point gets its ConvP from.
ConvP make_convp(int Nb, int C, int H, int W, int K, int R, int S, int stride,
                 int pad) {
  ConvP p{};
  p.Nb = Nb;
  p.C = C;
  p.H = H;
  p.W = W;
  p.K = K;
  p.R = p.Rf = R;
  p.S = p.Sf = S;
  p.str = stride;
  p.pad = pad;
  p.Ho = (p.H + 2 * pad - R) / stride + 1;
  p.Wo = (p.W + 2 * pad - S) / stride + 1;
  p.M = p.Nb * p.Ho * p.Wo;
  p.Kd = R * S * p.C;
  return g_tap_clip ? clip_taps(p) : p;
}

ConvP make_convp(const Tensor& x, int K, int R, int S, int stride, int pad) {
  return make_convp((int)x.size(0), (int)x.size(1), (int)x.size(2),
                    (int)x.size(3), K, R, S, stride, pad);
}

// ---------------------------------------------------------------- conv+BN --
std::vector<Tensor> conv_bn_act_fwd(
    Tensor x, Tensor w, Tensor gamma, Tensor beta, Tensor running_mean,
    Tensor running_var, int64_t stride, int64_t pad, double momentum,
    double eps, bool training, int64_t act,
    c10::optional<Tensor> residual, c10::optional<Tensor> stats_buf) {
  check_cl(x, "x");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
                  w.is_contiguous() && w.dim() == 4,
              "w must be contiguous bf16 KRSC");
  check_f32(gamma, "gamma");
  check_f32(beta, "beta");
  int K = (int)w.size(0), R = (int)w.size(1), S = (int)w.size(2);
  TORCH_CHECK(w.size(3) == x.size(1), "w in-channels mismatch");
  ConvP p = make_convp(x, K, R, S, (int)stride, (int)pad);

  Tensor convout = empty_cl_bf16(p.Nb, K, p.Ho, p.Wo, x);
  Tensor y = empty_cl_bf16(p.Nb, K, p.Ho, p.Wo, x);
  auto fopt = x.options().dtype(torch::kFloat32);
  Tensor stats, smean, sinvstd;
  float* stats_ptr = nullptr;
  if (training) {
    smean = at::empty({K}, fopt);
    sinvstd = at::empty({K}, fopt);
  } else {
    smean = at::empty({0}, fopt);
    sinvstd = at::empty({0}, fopt);
  }
  const void* res_ptr = nullptr;
  if (residual.has_value()) {
    check_cl(*residual, "residual");
    res_ptr = residual->data_ptr();
  }
  auto st = cur_stream();
  int splitk = conv_fwd_splitk(p);
  // the owner kernel keeps its sums in the workgroup: no stats buffer
  const int own = (training && splitk > 1)
                      ? bn_owner_fwd_pick((long)p.M, K, 0) : 0;
  if (training && !own) {
    // stats_buf (manager arena) arrives pre-zeroed by the fused optimizer
    stats = stats_buf.has_value() ? *stats_buf : at::zeros({2L * K}, fopt);
    stats_ptr = stats.data_ptr<float>();
  }
  if (splitk > 1) {
    int kchunk = ((p.Kd + splitk - 1) / splitk + 31) / 32 * 32;
    splitk = (p.Kd + kchunk - 1) / kchunk;
    // latency path: per-split f32 slabs -> stats reduce -> BN apply (+cast);
    // slabs are fully written by the conv grid, so no zeroing needed
    Tensor ws = at::empty({(long)splitk * p.M * K}, fopt);
    launch_conv_fwd_splitk(x.data_ptr(), w.data_ptr(), ws.data_ptr<float>(),
                           p, splitk, st);
    if (own) {
      // one workgroup per channel slice reduces and applies: no stats
      // arena, no atomics, one slab pass
      launch_bn_fwd_owner(ws.data_ptr<float>(), res_ptr, y.data_ptr(),
                          convout.data_ptr(), gamma.data_ptr<float>(),
                          beta.data_ptr<float>(),
                          running_mean.data_ptr<float>(),
                          running_var.data_ptr<float>(),
                          smean.data_ptr<float>(), sinvstd.data_ptr<float>(),
                          (long)p.M, K, (float)momentum, (float)eps,
                          (int)act, splitk, own, st);
      return {y, convout, smean, sinvstd};
    }
    if (training)
      launch_stats_reduce(ws.data_ptr<float>(), stats_ptr, (long)p.M, K,
                          splitk, st);
    launch_bn_apply_f32(ws.data_ptr<float>(), res_ptr, y.data_ptr(),
                        convout.data_ptr(), stats_ptr,
                        gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        running_mean.data_ptr<float>(),
                        running_var.data_ptr<float>(),
                        training ? smean.data_ptr<float>() : nullptr,
                        training ? sinvstd.data_ptr<float>() : nullptr,
                        (long)p.M, K, (float)momentum, (float)eps,
                        training ? 1 : 0, (int)act, splitk, st);
  } else {
    launch_conv_fwd(x.data_ptr(), w.data_ptr(), convout.data_ptr(),
                    g_deterministic ? nullptr : stats_ptr, p, st);
    if (g_deterministic && training)
      launch_stats_bf16_det(convout.data_ptr(), stats_ptr, (long)p.M, K,
                            st);
    launch_bn_apply(convout.data_ptr(), res_ptr, y.data_ptr(), stats_ptr,
                    gamma.data_ptr<float>(), beta.data_ptr<float>(),
                    running_mean.data_ptr<float>(),
                    running_var.data_ptr<float>(),
                    training ? smean.data_ptr<float>() : nullptr,
                    training ? sinvstd.data_ptr<float>() : nullptr,
                    (long)p.M, K, (float)momentum, (float)eps,
                    training ? 1 : 0, (int)act, st);
  }
  return {y, convout, smean, sinvstd};
}

// dx of one conv from its dz (`dconv`): the split decision, the dgrad
// launch, the slab sum and the optional fused upstream BN-backward sums
// (fuse_up, see conv_bn_act_bwd).  p is the FORWARD geometry of the conv.
//
// Weight layout: `w_rsck` absent, or the KRSC weight `w` itself, selects the
// KRSC-direct B path; any other tensor is taken as the permuted RSCK image
// and runs MODE 2 on it.  With dx_accum given, dgrad ACCUMULATES into it
// (dx_total = dx + residual-path grad without a separate add kernel).
Tensor dgrad_dx(const Tensor& dconv, const Tensor& w,
                const c10::optional<Tensor>& w_rsck, const ConvP& p,
                const c10::optional<Tensor>& dx_accum,
                const c10::optional<std::vector<Tensor>>& fuse_up,
                int up_mask_mode, hipStream_t st) {
  const bool krsc =
      !w_rsck.has_value() || w_rsck->data_ptr() == w.data_ptr();
  const Tensor& wt = krsc ? w : *w_rsck;
  TORCH_CHECK(wt.is_contiguous() && wt.scalar_type() == torch::kBFloat16,
              krsc ? "w must be contiguous bf16"
                   : "w_rsck must be contiguous bf16");
  TORCH_CHECK(wt.numel() == (int64_t)p.K * p.Rf * p.Sf * p.C,
              "dgrad weight has ", wt.numel(), " elements, expected K*R*S*C");
  auto fopt = dconv.options().dtype(torch::kFloat32);
  const int layout = krsc ? DGRAD_W_KRSC : DGRAD_W_RSCK;
  int accum = dx_accum.has_value() ? 1 : 0;
  Tensor dx = accum ? *dx_accum : empty_cl_bf16(p.Nb, p.C, p.H, p.W, dconv);
  ConvP pd = p;
  pd.M = p.Nb * p.H * p.W;
  pd.Kd = p.R * p.S * p.K;
  int splitk = conv_dgrad_splitk(p);
  const bool fuse = fuse_up.has_value();
  if (splitk > 1) {
    int kchunk = ((pd.Kd + splitk - 1) / splitk + 31) / 32 * 32;
    splitk = (pd.Kd + kchunk - 1) / kchunk;
    Tensor wsd = at::empty({(long)splitk * pd.M * p.C}, fopt);
    launch_conv_dgrad(dconv.data_ptr(), wt.data_ptr(), nullptr,
                      wsd.data_ptr<float>(), splitk, pd, 0, layout, st);
    if (fuse) {
      auto& f = *fuse_up;
      launch_cast_bnact(wsd.data_ptr<float>(), dx.data_ptr(), (long)pd.M,
                        p.C, splitk, accum, f[0].data_ptr(),
                        f[1].defined() ? f[1].data_ptr() : f[0].data_ptr(),
                        f[2].data_ptr<float>(), f[3].data_ptr<float>(),
                        f[4].data_ptr<float>(), f[5].data_ptr<float>(),
                        f[6].data_ptr<float>(), f[7].data_ptr<float>(),
                        up_mask_mode, st);
    } else {
      launch_cast_f32_bf16(wsd.data_ptr<float>(), dx.data_ptr(),
                           (long)pd.M * p.C, splitk, accum, st);
    }
  } else {
    launch_conv_dgrad(dconv.data_ptr(), wt.data_ptr(), dx.data_ptr(), nullptr,
                      1, pd, accum, layout, st);
    if (fuse) {
      auto& f = *fuse_up;
      launch_bnact_bwd_reduce(dx.data_ptr(), f[1].defined()
                                  ? f[1].data_ptr() : f[0].data_ptr(),
                              f[0].data_ptr(), f[2].data_ptr<float>(),
                              f[3].data_ptr<float>(),
                              f[4].data_ptr<float>(),
                              f[5].data_ptr<float>(),
                              f[6].data_ptr<float>(),
                              f[7].data_ptr<float>(), (long)pd.M, p.C,
                              up_mask_mode, st);
    }
  }
  return dx;
}

// Test/debug entry, the dgrad counterpart of wgrad_only: exactly the dx
// dispatch of conv_bn_act_bwd without the BN backward in front (whose
// channel sums are atomic-order dependent).  dz is the conv-output gradient
// [Nb,K,Ho,Wo], w the KRSC weight, H/W the input size.
Tensor conv_dgrad_only(Tensor dz, Tensor w, int64_t H, int64_t W,
                       int64_t stride, int64_t pad,
                       c10::optional<Tensor> w_rsck,
                       c10::optional<Tensor> dx_accum) {
  check_cl(dz, "dz");
  TORCH_CHECK(w.dim() == 4 && w.size(0) == dz.size(1),
              "w must be [K,R,S,C] with K = dz channels");
  const ConvP p = make_convp((int)dz.size(0), (int)w.size(3), (int)H, (int)W,
                             (int)w.size(0), (int)w.size(1), (int)w.size(2),
                             (int)stride, (int)pad);
  TORCH_CHECK(dz.size(2) == p.Ho && dz.size(3) == p.Wo,
              "dz spatial size does not match H, W, stride, pad");
  if (dx_accum.has_value()) {
    check_cl(*dx_accum, "dx_accum");
    TORCH_CHECK(dx_accum->size(0) == p.Nb && dx_accum->size(1) == p.C &&
                    dx_accum->size(2) == p.H && dx_accum->size(3) == p.W,
                "dx_accum must be [Nb,C,H,W]");
  }
  return dgrad_dx(dz, w, w_rsck, p, dx_accum, c10::nullopt, 0, cur_stream());
}

std::vector<Tensor> conv_bn_act_bwd(
    Tensor dy, Tensor y, Tensor x, Tensor w, c10::optional<Tensor> w_rsck,
    Tensor convout,
    Tensor gamma, Tensor beta, Tensor save_mean, Tensor save_invstd,
    int64_t stride, int64_t pad, int64_t act, bool need_dx, bool has_res,
    c10::optional<Tensor> dw_out, c10::optional<Tensor> dgamma_out,
    c10::optional<Tensor> dbeta_out, c10::optional<Tensor> dx_accum,
    c10::optional<std::vector<Tensor>> fuse_up, int64_t up_mask_mode,
    bool sums_ready, c10::optional<Tensor> sum_dz_in,
    c10::optional<Tensor> sum_dzx_in) {
  // fuse_up = [x_up, y_up, smean_up, sinvstd_up, gamma_up, beta_up,
  //            sum_dz_up, sum_dzx_up]: while producing dx (= the UPSTREAM
  //            conv's dy), also complete that conv's BN-backward channel
  //            sums — fused into the slab-sum cast when dgrad is split-K,
  //            else run as the standalone reduce right after dgrad.  The
  //            upstream conv's own backward then passes sums_ready=true
  //            (with sum_dz_in/sum_dzx_in in non-direct-grad mode) and
  //            skips its reduce pass.
  // Direct-grad mode: when dw_out/dgamma_out/dbeta_out are given they are
  // PRE-ZEROED flat .grad views — the kernels accumulate straight into
  // them, skipping autograd's per-parameter accumulate pass.
  check_cl(dy, "dy");
  check_cl(y, "y");
  check_cl(x, "x");
  check_cl(convout, "convout");
  int K = (int)w.size(0), R = (int)w.size(1), S = (int)w.size(2);
  ConvP p = make_convp(x, K, R, S, (int)stride, (int)pad);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto st = cur_stream();

  bool direct = dw_out.has_value();
  // ReLU-mask source: residual epilogue needs y; otherwise the mask is
  // recovered from convout via BN algebra and y is never read
  int mask_mode = act == 1 ? (has_res ? 1 : 2)
                 : act == 2 ? (has_res ? 3 : 4) : 0;
  Tensor sum_dz, sum_dzx;
  const int own = sums_ready ? 0 : bn_owner_bwd_pick((long)p.M, K, 0);
  if (sums_ready) {  // computed by the downstream conv's dx producer
    sum_dz = direct ? *dbeta_out : *sum_dz_in;
    sum_dzx = direct ? *dgamma_out : *sum_dzx_in;
  } else {
    sum_dz = direct ? *dbeta_out : at::zeros({K}, fopt);
    sum_dzx = direct ? *dgamma_out : at::zeros({K}, fopt);
    if (!own)
      launch_bnact_bwd_reduce(dy.data_ptr(), y.data_ptr(),
                              convout.data_ptr(),
                              save_mean.data_ptr<float>(),
                              save_invstd.data_ptr<float>(),
                              gamma.data_ptr<float>(),
                              beta.data_ptr<float>(),
                              sum_dz.data_ptr<float>(),
                              sum_dzx.data_ptr<float>(),
                              (long)p.M, K, mask_mode, st);
  }

  Tensor dconv = empty_cl_bf16(p.Nb, K, p.Ho, p.Wo, x);
  Tensor dres;
  void* dres_ptr = nullptr;
  if (has_res) {
    dres = empty_cl_bf16(p.Nb, K, p.Ho, p.Wo, x);
    dres_ptr = dres.data_ptr();
  }
  if (own)  // channel sums + apply in one launch (read-add-write sums)
    launch_bn_bwd_owner(dy.data_ptr(), y.data_ptr(), convout.data_ptr(),
                        save_mean.data_ptr<float>(),
                        save_invstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        sum_dz.data_ptr<float>(), sum_dzx.data_ptr<float>(),
                        dconv.data_ptr(), dres_ptr, (long)p.M, K, mask_mode,
                        own, st);
  else
    launch_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), convout.data_ptr(),
                        save_mean.data_ptr<float>(),
                        save_invstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        sum_dz.data_ptr<float>(), sum_dzx.data_ptr<float>(),
                        dconv.data_ptr(), dres_ptr, (long)p.M, K, mask_mode,
                        st);

  Tensor dw = direct ? *dw_out
                     : at::zeros({(int64_t)K, R, S, (int64_t)p.C}, fopt);
  if (direct) record_tap_window(dw, p);
  if (direct && g_wgrad_defer) {
    g_pending.push_back({x, dconv, dw, p});  // runs batched at flush_wgrad
  } else {
    int msplit = wgrad_msplit(p);
    Tensor ws;
    float* ws_ptr = nullptr;
    if (msplit > 1) {
      ws = at::empty({(long)msplit * K * p.Kd}, fopt);
      ws_ptr = ws.data_ptr<float>();
    }
    launch_wgrad(x.data_ptr(), dconv.data_ptr(), dw.data_ptr<float>(), ws_ptr,
                 p, (int)g_wgrad_tr, st);
  }

  TORCH_CHECK(need_dx || !fuse_up.has_value(),
              "fuse_up requires need_dx (the fused reduce rides the dx "
              "production)");
  Tensor dx;
  if (need_dx)
    dx = dgrad_dx(dconv, w, w_rsck, p, dx_accum, fuse_up, (int)up_mask_mode,
                  st);
  // dgamma = Σ dz·xhat, dbeta = Σ dz
  return {dx, dw, sum_dzx, sum_dz, dres};
}

// --------------------------------------------------------- depthwise conv --
// The depthwise kernels keep the filter taps in a register array of
// DW_MAXRS = 25 floats (elem_kernels.hip): a larger filter would index
// past it, so it is refused here, before any launch.
void check_dw_geometry(int R, int S, int64_t stride, int H, int W,
                       int64_t pad) {
  TORCH_CHECK(R >= 1 && S >= 1 && R * S <= 25,
              "depthwise filter must have R*S <= 25 taps, got ", R, "x", S);
  TORCH_CHECK(stride >= 1, "depthwise stride must be >= 1, got ", stride);
  TORCH_CHECK(pad >= 0, "depthwise pad must be >= 0, got ", pad);
  TORCH_CHECK(H + 2 * pad >= R && W + 2 * pad >= S,
              "depthwise output must be at least 1x1: input ", H, "x", W,
              ", pad ", pad, ", filter ", R, "x", S);
}

std::vector<Tensor> dw_conv_bn_fwd(
    Tensor x, Tensor w, Tensor gamma, Tensor beta, Tensor running_mean,
    Tensor running_var, int64_t stride, int64_t pad, double momentum,
    double eps, bool training, int64_t act, c10::optional<Tensor> residual) {
  check_cl(x, "x");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
                  w.is_contiguous() && w.dim() == 3,
              "w must be contiguous bf16 [R,S,C]");
  int Nb = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2),
      W = (int)x.size(3);
  int R = (int)w.size(0), S = (int)w.size(1);
  TORCH_CHECK((int)w.size(2) == C, "depthwise channel mismatch");
  check_dw_geometry(R, S, stride, H, W, pad);
  int Ho = (H + 2 * (int)pad - R) / (int)stride + 1;
  int Wo = (W + 2 * (int)pad - S) / (int)stride + 1;
  long M = (long)Nb * Ho * Wo;
  auto fopt = x.options().dtype(torch::kFloat32);
  Tensor convout = empty_cl_bf16(Nb, C, Ho, Wo, x);
  Tensor y = empty_cl_bf16(Nb, C, Ho, Wo, x);
  Tensor stats, smean, sinvstd;
  float* stats_ptr = nullptr;
  if (training) {
    stats = at::zeros({2L * C}, fopt);
    smean = at::empty({C}, fopt);
    sinvstd = at::empty({C}, fopt);
    stats_ptr = stats.data_ptr<float>();
  } else {
    smean = at::empty({0}, fopt);
    sinvstd = at::empty({0}, fopt);
  }
  const void* res_ptr = nullptr;
  if (residual.has_value()) {
    check_cl(*residual, "residual");
    res_ptr = residual->data_ptr();
  }
  auto st = cur_stream();
  launch_dw_fwd(x.data_ptr(), w.data_ptr(), convout.data_ptr(),
                g_deterministic ? nullptr : stats_ptr, Nb, H, W, C, Ho, Wo,
                R, S, (int)stride, (int)pad, st);
  if (g_deterministic && training)
    launch_stats_bf16_det(convout.data_ptr(), stats_ptr, M, C, st);
  launch_bn_apply(convout.data_ptr(), res_ptr, y.data_ptr(), stats_ptr,
                  gamma.data_ptr<float>(), beta.data_ptr<float>(),
                  running_mean.data_ptr<float>(),
                  running_var.data_ptr<float>(),
                  training ? smean.data_ptr<float>() : nullptr,
                  training ? sinvstd.data_ptr<float>() : nullptr, M, C,
                  (float)momentum, (float)eps, training ? 1 : 0, (int)act,
                  st);
  return {y, convout, smean, sinvstd};
}

std::vector<Tensor> dw_conv_bn_bwd(
    Tensor dy, Tensor y, Tensor x, Tensor w, Tensor convout, Tensor gamma,
    Tensor beta, Tensor save_mean, Tensor save_invstd, int64_t stride,
    int64_t pad, int64_t act, bool need_dx, bool has_res) {
  check_cl(dy, "dy");
  check_cl(x, "x");
  int Nb = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2),
      W = (int)x.size(3);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 &&
                  w.is_contiguous() && w.dim() == 3 && w.size(2) == C,
              "w must be contiguous bf16 [R,S,C] with C = x channels");
  int R = (int)w.size(0), S = (int)w.size(1);
  check_dw_geometry(R, S, stride, H, W, pad);
  int Ho = (int)dy.size(2), Wo = (int)dy.size(3);
  TORCH_CHECK(dy.size(0) == Nb && dy.size(1) == C &&
                  Ho == (H + 2 * (int)pad - R) / (int)stride + 1 &&
                  Wo == (W + 2 * (int)pad - S) / (int)stride + 1,
              "dy shape does not match the depthwise output of x");
  long M = (long)Nb * Ho * Wo;
  auto fopt = x.options().dtype(torch::kFloat32);
  auto st = cur_stream();
  int mask_mode = act == 1 ? (has_res ? 1 : 2)
                 : act == 2 ? (has_res ? 3 : 4) : 0;
  Tensor sum_dz = at::zeros({C}, fopt);
  Tensor sum_dzx = at::zeros({C}, fopt);
  launch_bnact_bwd_reduce(dy.data_ptr(), y.data_ptr(), convout.data_ptr(),
                          save_mean.data_ptr<float>(),
                          save_invstd.data_ptr<float>(),
                          gamma.data_ptr<float>(), beta.data_ptr<float>(),
                          sum_dz.data_ptr<float>(), sum_dzx.data_ptr<float>(),
                          M, C, mask_mode, st);
  Tensor dconv = empty_cl_bf16(Nb, C, Ho, Wo, x);
  Tensor dres;
  void* dres_ptr = nullptr;
  if (has_res) {
    dres = empty_cl_bf16(Nb, C, Ho, Wo, x);
    dres_ptr = dres.data_ptr();
  }
  launch_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), convout.data_ptr(),
                      save_mean.data_ptr<float>(),
                      save_invstd.data_ptr<float>(), gamma.data_ptr<float>(),
                      beta.data_ptr<float>(), sum_dz.data_ptr<float>(),
                      sum_dzx.data_ptr<float>(), dconv.data_ptr(), dres_ptr,
                      M, C, mask_mode, st);
  Tensor dw = at::zeros({(int64_t)R, (int64_t)S, (int64_t)C}, fopt);
  launch_dw_wgrad(x.data_ptr(), dconv.data_ptr(), dw.data_ptr<float>(), Nb,
                  H, W, C, Ho, Wo, R, S, (int)stride, (int)pad, st);
  Tensor dx;
  if (need_dx) {
    dx = empty_cl_bf16(Nb, C, H, W, x);
    launch_dw_dgrad(dconv.data_ptr(), w.data_ptr(), dx.data_ptr(), Nb, H, W,
                    C, Ho, Wo, R, S, (int)stride, (int)pad, st);
  }
  return {dx, dw, sum_dzx, sum_dz, dres};
}

// ----------------------------------------------------------------- pools --
std::vector<Tensor> maxpool_fwd(Tensor x) {
  check_cl(x, "x");
  int Nb = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2),
      W = (int)x.size(3);
  int Hp = (H + 2 - 3) / 2 + 1, Wp = (W + 2 - 3) / 2 + 1;
  Tensor y = empty_cl_bf16(Nb, C, Hp, Wp, x);
  Tensor idx = at::empty({Nb, Hp, Wp, C}, x.options().dtype(torch::kUInt8));
  launch_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr<unsigned char>(),
                     Nb, H, W, C, Hp, Wp, cur_stream());
  return {y, idx};
}

Tensor maxpool_bwd(Tensor dy, Tensor idx, int64_t H, int64_t W) {
  check_cl(dy, "dy");
  int Nb = (int)dy.size(0), C = (int)dy.size(1), Hp = (int)dy.size(2),
      Wp = (int)dy.size(3);
  Tensor dx = empty_cl_bf16(Nb, C, H, W, dy);
  launch_maxpool_bwd(dy.data_ptr(), idx.data_ptr<unsigned char>(),
                     dx.data_ptr(), Nb, (int)H, (int)W, C, Hp, Wp,
                     cur_stream());
  return dx;
}

Tensor avgpool_fwd(Tensor x) {
  check_cl(x, "x");
  int Nb = (int)x.size(0), C = (int)x.size(1);
  int HW = (int)(x.size(2) * x.size(3));
  Tensor y = at::empty({Nb, C}, x.options());
  launch_avgpool_fwd(x.data_ptr(), y.data_ptr(), Nb, HW, C, cur_stream());
  return y;
}

Tensor avgpool_bwd(Tensor dy, int64_t H, int64_t W) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() &&
              dy.scalar_type() == torch::kBFloat16);
  int Nb = (int)dy.size(0), C = (int)dy.size(1);
  Tensor dx = empty_cl_bf16(Nb, C, H, W, dy);
  launch_avgpool_bwd(dy.data_ptr(), dx.data_ptr(), Nb, (int)(H * W), C,
                     cur_stream());
  return dx;
}

// -------------------------------------------------------------- classifier --
Tensor linear_fwd(Tensor x, Tensor w, c10::optional<Tensor> bias) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                  w.scalar_type() == torch::kBFloat16,
              "w must be contiguous bf16 on GPU");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2,
              "linear_fwd: x must be [B, In] and w [Out, In], got ", x.dim(),
              "-D x and ", w.dim(), "-D w");
  int B = (int)x.size(0), In = (int)x.size(1), Out = (int)w.size(0);
  TORCH_CHECK(w.size(1) == In, "linear_fwd: w has ", w.size(1),
              " input columns, x has ", In);
  // k_linear_fwd reads x and w as vec8 chunks, at most 4 per lane
  TORCH_CHECK(In % 8 == 0, "linear_fwd: In must be a multiple of 8, got ",
              In);
  TORCH_CHECK(In <= 2048, "linear_fwd: In must be <= 2048, got ", In);
  Tensor y = at::empty({B, Out}, x.options().dtype(torch::kFloat32));
  const float* bptr = nullptr;
  if (bias.has_value()) {
    check_f32(*bias, "bias");
    TORCH_CHECK(bias->numel() == Out, "linear_fwd: bias has ", bias->numel(),
                " elements, Out is ", Out);
    bptr = bias->data_ptr<float>();
  }
  launch_linear_fwd(x.data_ptr(), w.data_ptr(), bptr, y.data_ptr<float>(), B,
                    In, Out, cur_stream());
  return y;
}

std::vector<Tensor> linear_bwd(Tensor dy, Tensor x, Tensor w, bool need_dx,
                               bool need_db, c10::optional<Tensor> dw_out,
                               c10::optional<Tensor> db_out) {
  check_f32(dy, "dy");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kBFloat16 && x.dim() == 2,
              "linear_bwd: x must be contiguous bf16 [B, In] on GPU");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() &&
                  w.scalar_type() == torch::kBFloat16 && w.dim() == 2,
              "linear_bwd: w must be contiguous bf16 [Out, In] on GPU");
  int B = (int)x.size(0), In = (int)x.size(1), Out = (int)w.size(0);
  TORCH_CHECK(w.size(1) == In, "linear_bwd: w has ", w.size(1),
              " input columns, x has ", In);
  TORCH_CHECK(dy.dim() == 2 && dy.size(0) == B && dy.size(1) == Out,
              "linear_bwd: dy must be [B, Out] = [", B, ", ", Out, "]");
  if (dw_out.has_value()) {
    check_f32(*dw_out, "dw_out");
    TORCH_CHECK(dw_out->dim() == 2 && dw_out->size(0) == Out &&
                    dw_out->size(1) == In,
                "linear_bwd: dw_out must be [Out, In] = [", Out, ", ", In,
                "]");
  }
  if (db_out.has_value()) {
    check_f32(*db_out, "db_out");
    TORCH_CHECK(db_out->numel() == Out, "linear_bwd: db_out has ",
                db_out->numel(), " elements, Out is ", Out);
  }
  auto fopt = x.options().dtype(torch::kFloat32);
  bool direct = dw_out.has_value();
  Tensor dx, dw = direct ? *dw_out : at::empty({Out, In}, fopt);
  Tensor db = direct ? (db_out.has_value() ? *db_out : Tensor())
                     : (need_db ? at::empty({Out}, fopt) : Tensor());
  void* dx_ptr = nullptr;
  if (need_dx) {
    dx = at::empty({B, In}, x.options());
    dx_ptr = dx.data_ptr();
  }
  launch_linear_bwd(dy.data_ptr<float>(), x.data_ptr(), w.data_ptr(), dx_ptr,
                    dw.data_ptr<float>(),
                    db.defined() ? db.data_ptr<float>() : nullptr, B, In, Out,
                    direct ? 1 : 0, cur_stream());
  return {dx, dw, db};
}

std::vector<Tensor> cross_entropy_fwd_bwd(Tensor logits, Tensor target) {
  check_f32(logits, "logits");
  TORCH_CHECK(target.scalar_type() == torch::kLong && target.is_contiguous());
  int B = (int)logits.size(0), NC = (int)logits.size(1);
  Tensor loss = at::zeros({}, logits.options());
  Tensor dlogits = at::empty({B, NC}, logits.options());
  launch_ce_fwd_bwd(logits.data_ptr<float>(), target.data_ptr<long>(),
                    loss.data_ptr<float>(), dlogits.data_ptr<float>(), B, NC,
                    cur_stream());
  return {loss, dlogits};
}

// Label-smoothed form; eps == 0 launches the one-hot kernels above.
std::vector<Tensor> cross_entropy_ls_fwd_bwd(Tensor logits, Tensor target,
                                             double eps) {
  if (eps == 0.0) return cross_entropy_fwd_bwd(logits, target);
  TORCH_CHECK(eps > 0.0 && eps <= 1.0,
              "label_smoothing must be in [0, 1], got ", eps);
  check_f32(logits, "logits");
  TORCH_CHECK(target.scalar_type() == torch::kLong && target.is_contiguous());
  int B = (int)logits.size(0), NC = (int)logits.size(1);
  Tensor loss = at::zeros({}, logits.options());
  Tensor dlogits = at::empty({B, NC}, logits.options());
  launch_ce_ls_fwd_bwd(logits.data_ptr<float>(), target.data_ptr<long>(),
                       loss.data_ptr<float>(), dlogits.data_ptr<float>(), B,
                       NC, (float)eps, cur_stream());
  return {loss, dlogits};
}

// ------------------------------------------------------------------ gemm ---
Tensor gemm_bf16(Tensor a, Tensor b) {
  // C[M,N] = A[M,K] · B[N,K]^T
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() &&
              a.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(b.is_contiguous() && b.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(a.size(1) == b.size(1), "K mismatch");
  int M = (int)a.size(0), K = (int)a.size(1), N = (int)b.size(0);
  Tensor c = at::empty({M, N}, a.options());
  launch_gemm_bf16(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K,
                   cur_stream());
  return c;
}

// Debug/test entry: standalone weight-gradient (immediate or deferred).
Tensor wgrad_only(Tensor x, Tensor dz, int64_t K, int64_t R, int64_t S,
                  int64_t stride, int64_t pad, bool defer,
                  c10::optional<Tensor> dw_out) {
  check_cl(x, "x");
  check_cl(dz, "dz");
  ConvP p = make_convp(x, (int)K, (int)R, (int)S, (int)stride, (int)pad);
  Tensor dw = dw_out.has_value()
                  ? *dw_out
                  : at::zeros({K, R, S, (int64_t)p.C},
                              x.options().dtype(torch::kFloat32));
  if (defer) {
    g_pending.push_back({x, dz, dw, p});
  } else {
    int msplit = wgrad_msplit(p);
    Tensor ws;
    float* ws_ptr = nullptr;
    if (msplit > 1) {
      ws = at::empty({(long)msplit * p.K * p.Kd},
                     x.options().dtype(torch::kFloat32));
      ws_ptr = ws.data_ptr<float>();
    }
    launch_wgrad(x.data_ptr(), dz.data_ptr(), dw.data_ptr<float>(), ws_ptr,
                 p, (int)g_wgrad_tr, cur_stream());
  }
  return dw;
}

// ------------------------------------------------------------- optimizers --
// probe_prev/probe_sumsq/probe_out (all-or-none): fused grad-divergence
// probe — Σ(g−prev)² accumulated in-kernel, sqrt appended to probe_out.
void adam_step(Tensor master, Tensor grad, Tensor m, Tensor v,
               c10::optional<Tensor> shadow, Tensor step_t, double lr,
               double b1, double b2, double eps, double wd, bool zero_grad,
               c10::optional<Tensor> extra_zero,
               c10::optional<Tensor> grad_bf16, double grad_scale,
               c10::optional<Tensor> probe_prev,
               c10::optional<Tensor> probe_sumsq,
               c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  launch_adam_step(master.data_ptr<float>(), grad.data_ptr<float>(),
                   m.data_ptr<float>(), v.data_ptr<float>(),
                   opt_ptr(shadow), step_t.data_ptr<float>(),
                   master.numel(), (float)lr, (float)b1, (float)b2,
                   (float)eps, (float)wd, zero_grad ? 1 : 0,
                   opt_ptr<float>(extra_zero),
                   extra_zero.has_value() ? extra_zero->numel() : 0,
                   opt_ptr(grad_bf16), (float)grad_scale,
                   opt_ptr<float>(probe_prev), opt_ptr<float>(probe_sumsq),
                   opt_ptr<float>(probe_out), cur_stream());
}

void sgd_step(Tensor master, Tensor grad, c10::optional<Tensor> mom,
              c10::optional<Tensor> shadow, double lr, double mu, double wd,
              bool zero_grad, c10::optional<Tensor> grad_bf16,
              double grad_scale, c10::optional<Tensor> probe_prev,
              c10::optional<Tensor> probe_sumsq,
              c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  launch_sgd_step(master.data_ptr<float>(), grad.data_ptr<float>(),
                  opt_ptr<float>(mom), opt_ptr(shadow), master.numel(),
                  (float)lr, (float)mu, (float)wd, zero_grad ? 1 : 0,
                  opt_ptr(grad_bf16), (float)grad_scale,
                  opt_ptr<float>(probe_prev), opt_ptr<float>(probe_sumsq),
                  opt_ptr<float>(probe_out), cur_stream());
}

// Scheduled / extended forms (adam_step / sgd_step above are untouched and
// keep launching k_adam_step / k_sgd_step).
// lr_table (optional): f32 [T] on the GPU; the kernel reads
// lr_table[min(step_t − 1, T − 1)] after the counter bump, so `lr` is only
// used without a table.  lr_out (optional): f32 [1], receives the lr used.
const float* sched_table(const c10::optional<Tensor>& lr_table,
                         const Tensor& master, long* T) {
  *T = 0;
  if (!lr_table.has_value()) return nullptr;
  check_f32(*lr_table, "lr_table");
  TORCH_CHECK(lr_table->dim() == 1 && lr_table->numel() >= 1
                  && lr_table->device() == master.device(),
              "lr_table must be a non-empty 1-D tensor on master's device");
  *T = lr_table->numel();
  return lr_table->data_ptr<float>();
}

float* sched_scalar(const c10::optional<Tensor>& t, const Tensor& master,
                    const char* name) {
  if (!t.has_value()) return nullptr;
  check_f32(*t, name);
  TORCH_CHECK(t->numel() == 1 && t->device() == master.device(), name,
              " must hold one element on master's device");
  return t->data_ptr<float>();
}

void adam_step_sched(Tensor master, Tensor grad, Tensor m, Tensor v,
                     c10::optional<Tensor> shadow, Tensor step_t,
                     c10::optional<Tensor> lr_table,
                     c10::optional<Tensor> lr_out, double lr, double b1,
                     double b2, double eps, double wd, bool decoupled,
                     bool zero_grad, c10::optional<Tensor> extra_zero,
                     c10::optional<Tensor> grad_bf16, double grad_scale,
                     c10::optional<Tensor> probe_prev,
                     c10::optional<Tensor> probe_sumsq,
                     c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel() && m.numel() == master.numel()
                  && v.numel() == master.numel(),
              "grad / m / v must match master's size");
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_adam_step_ex(master.data_ptr<float>(), grad.data_ptr<float>(),
                      m.data_ptr<float>(), v.data_ptr<float>(),
                      opt_ptr(shadow), st, master.numel(), (float)lr,
                      (float)b1, (float)b2, (float)eps, (float)wd,
                      zero_grad ? 1 : 0, opt_ptr<float>(extra_zero),
                      extra_zero.has_value() ? extra_zero->numel() : 0,
                      opt_ptr(grad_bf16), (float)grad_scale,
                      opt_ptr<float>(probe_prev),
                      opt_ptr<float>(probe_sumsq), opt_ptr<float>(probe_out),
                      table, T, out, decoupled ? 1 : 0, cur_stream());
}

void sgd_step_sched(Tensor master, Tensor grad, c10::optional<Tensor> mom,
                    c10::optional<Tensor> shadow,
                    c10::optional<Tensor> step_t,
                    c10::optional<Tensor> lr_table,
                    c10::optional<Tensor> lr_out, double lr, double mu,
                    double wd, bool nesterov, bool zero_grad,
                    c10::optional<Tensor> grad_bf16, double grad_scale,
                    c10::optional<Tensor> probe_prev,
                    c10::optional<Tensor> probe_sumsq,
                    c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel()
                  && (!mom.has_value() || mom->numel() == master.numel()),
              "grad / mom must match master's size");
  TORCH_CHECK(!nesterov || (mom.has_value() && mu > 0.0),
              "nesterov needs a momentum buffer and momentum > 0");
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  TORCH_CHECK(table == nullptr || step_t.has_value(),
              "lr_table needs the step_t device counter");
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_sgd_step_ex(master.data_ptr<float>(), grad.data_ptr<float>(),
                     opt_ptr<float>(mom), opt_ptr(shadow), master.numel(),
                     (float)lr, (float)mu, (float)wd, zero_grad ? 1 : 0,
                     opt_ptr(grad_bf16), (float)grad_scale,
                     opt_ptr<float>(probe_prev), opt_ptr<float>(probe_sumsq),
                     opt_ptr<float>(probe_out), st, table, T, out,
                     nesterov ? 1 : 0, cur_stream());
}

// Segmented forms.  chunks int32 [nchunks,3] = (segment, start, length) and
// seg_meta int32 [nseg,3] = (chunk begin, chunk end, flags) come from
// engine/flat.build_segment_table, which is correct by construction; the
// device tables are not re-read here.  seg_mul f32 [nseg,2].
struct SegTable {
  const int* chunks;
  int nchunks;
  const float* seg_mul;
  int nseg;
};

SegTable seg_table(const Tensor& chunks, const Tensor& seg_mul,
                   const Tensor& master) {
  TORCH_CHECK(chunks.scalar_type() == torch::kInt32 && chunks.dim() == 2
                  && chunks.size(1) == 3 && chunks.size(0) >= 1
                  && chunks.is_contiguous()
                  && chunks.device() == master.device(),
              "chunks must be a contiguous int32 [nchunks,3] tensor on "
              "master's device");
  check_f32(seg_mul, "seg_mul");
  TORCH_CHECK(seg_mul.dim() == 2 && seg_mul.size(1) == 2
                  && seg_mul.size(0) >= 1 && seg_mul.is_contiguous()
                  && seg_mul.device() == master.device(),
              "seg_mul must be a contiguous f32 [nseg,2] tensor on master's "
              "device");
  return {chunks.data_ptr<int>(), (int)chunks.size(0),
          seg_mul.data_ptr<float>(), (int)seg_mul.size(0)};
}

void seg_norms(Tensor master, Tensor grad, Tensor chunks, Tensor seg_meta,
               Tensor partials, Tensor seg_norms_out, Tensor seg_mul,
               Tensor norm_out, double wd, double max_norm, bool lars,
               double eta, c10::optional<Tensor> grad_bf16,
               double grad_scale) {
  check_f32(master, "master");
  check_f32(grad, "grad");
  check_f32(partials, "partials");
  check_f32(seg_norms_out, "seg_norms");
  check_f32(norm_out, "norm_out");
  SegTable t = seg_table(chunks, seg_mul, master);
  TORCH_CHECK(grad.numel() == master.numel(), "grad must match master");
  TORCH_CHECK(seg_meta.scalar_type() == torch::kInt32
                  && seg_meta.is_contiguous() && seg_meta.dim() == 2
                  && seg_meta.size(0) == t.nseg && seg_meta.size(1) == 3
                  && seg_meta.device() == master.device(),
              "seg_meta must be a contiguous int32 [nseg,3] tensor on "
              "master's device");
  TORCH_CHECK(partials.numel() == 2L * t.nchunks
                  && seg_norms_out.numel() == 2L * t.nseg
                  && norm_out.numel() == 2 && partials.is_contiguous()
                  && seg_norms_out.is_contiguous()
                  && partials.device() == master.device()
                  && seg_norms_out.device() == master.device()
                  && norm_out.device() == master.device(),
              "partials [nchunks,2], seg_norms [nseg,2], norm_out [2] on "
              "master's device");
  TORCH_CHECK(!grad_bf16.has_value()
                  || (grad_bf16->scalar_type() == torch::kBFloat16
                      && grad_bf16->numel() == master.numel()),
              "grad_bf16 must be a bf16 tensor of master's size");
  // the kernel's 16-byte vector loads index from these bases
  TORCH_CHECK((uintptr_t)master.data_ptr() % 16 == 0
                  && (uintptr_t)grad.data_ptr() % 16 == 0
                  && (!grad_bf16.has_value()
                      || (uintptr_t)grad_bf16->data_ptr() % 16 == 0),
              "master / grad / grad_bf16 must be 16-byte aligned");
  launch_seg_norms(master.data_ptr<float>(), grad.data_ptr<float>(),
                   opt_ptr(grad_bf16), (float)grad_scale, t.chunks,
                   t.nchunks, seg_meta.data_ptr<int>(), t.nseg,
                   partials.data_ptr<float>(),
                   seg_norms_out.data_ptr<float>(),
                   seg_mul.data_ptr<float>(), norm_out.data_ptr<float>(),
                   (float)wd, (float)max_norm, lars ? 1 : 0, (float)eta,
                   cur_stream());
}

void adam_step_seg(Tensor master, Tensor grad, Tensor m, Tensor v,
                   c10::optional<Tensor> shadow, Tensor step_t,
                   c10::optional<Tensor> lr_table,
                   c10::optional<Tensor> lr_out, double lr, double b1,
                   double b2, double eps, bool decoupled, bool zero_grad,
                   Tensor chunks, Tensor seg_mul,
                   c10::optional<Tensor> extra_zero,
                   c10::optional<Tensor> grad_bf16, double grad_scale,
                   c10::optional<Tensor> probe_prev,
                   c10::optional<Tensor> probe_sumsq,
                   c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel() && m.numel() == master.numel()
                  && v.numel() == master.numel(),
              "grad / m / v must match master's size");
  SegTable t = seg_table(chunks, seg_mul, master);
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_adam_step_seg(master.data_ptr<float>(), grad.data_ptr<float>(),
                       m.data_ptr<float>(), v.data_ptr<float>(),
                       opt_ptr(shadow), st, (float)lr, (float)b1, (float)b2,
                       (float)eps, zero_grad ? 1 : 0,
                       opt_ptr<float>(extra_zero),
                       extra_zero.has_value() ? extra_zero->numel() : 0,
                       opt_ptr(grad_bf16), (float)grad_scale,
                       opt_ptr<float>(probe_prev),
                       opt_ptr<float>(probe_sumsq), opt_ptr<float>(probe_out),
                       table, T, out, decoupled ? 1 : 0, t.chunks, t.nchunks,
                       t.seg_mul, cur_stream());
}

void sgd_step_seg(Tensor master, Tensor grad, c10::optional<Tensor> mom,
                  c10::optional<Tensor> shadow, c10::optional<Tensor> step_t,
                  c10::optional<Tensor> lr_table,
                  c10::optional<Tensor> lr_out, double lr, double mu,
                  bool nesterov, bool zero_grad, Tensor chunks,
                  Tensor seg_mul, c10::optional<Tensor> grad_bf16,
                  double grad_scale, c10::optional<Tensor> probe_prev,
                  c10::optional<Tensor> probe_sumsq,
                  c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel()
                  && (!mom.has_value() || mom->numel() == master.numel()),
              "grad / mom must match master's size");
  TORCH_CHECK(!nesterov || (mom.has_value() && mu > 0.0),
              "nesterov needs a momentum buffer and momentum > 0");
  SegTable t = seg_table(chunks, seg_mul, master);
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  TORCH_CHECK(table == nullptr || step_t.has_value(),
              "lr_table needs the step_t device counter");
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_sgd_step_seg(master.data_ptr<float>(), grad.data_ptr<float>(),
                      opt_ptr<float>(mom), opt_ptr(shadow), (float)lr,
                      (float)mu, zero_grad ? 1 : 0, opt_ptr(grad_bf16),
                      (float)grad_scale, opt_ptr<float>(probe_prev),
                      opt_ptr<float>(probe_sumsq), opt_ptr<float>(probe_out),
                      st, table, T, out, nesterov ? 1 : 0, t.chunks,
                      t.nchunks, t.seg_mul, cur_stream());
}

// Live-range forms: the unsegmented step with weight decay 0 over the chunks
// of `live` only.  live int32 [nchunks,4] = (start, run_len, run_pitch,
// nruns) comes from engine/flat.build_live_chunks, which checks every chunk
// against the buffer size on the host before the table is uploaded; the
// device table is not re-read here.
const int* live_table(const Tensor& live, const Tensor& master,
                      int* nchunks) {
  TORCH_CHECK(live.scalar_type() == torch::kInt32 && live.dim() == 2
                  && live.size(1) == 4 && live.size(0) >= 1
                  && live.is_contiguous()
                  && live.device() == master.device()
                  && (uintptr_t)live.data_ptr() % 16 == 0,
              "live must be a contiguous, 16-byte aligned int32 [nchunks,4] "
              "tensor on master's device");
  *nchunks = (int)live.size(0);
  return live.data_ptr<int>();
}

void adam_step_live(Tensor master, Tensor grad, Tensor m, Tensor v,
                    c10::optional<Tensor> shadow, Tensor step_t,
                    c10::optional<Tensor> lr_table,
                    c10::optional<Tensor> lr_out, double lr, double b1,
                    double b2, double eps, bool zero_grad, Tensor live,
                    c10::optional<Tensor> extra_zero,
                    c10::optional<Tensor> grad_bf16, double grad_scale,
                    c10::optional<Tensor> probe_prev,
                    c10::optional<Tensor> probe_sumsq,
                    c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel() && m.numel() == master.numel()
                  && v.numel() == master.numel(),
              "grad / m / v must match master's size");
  int nchunks = 0;
  const int* chunks = live_table(live, master, &nchunks);
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_adam_step_live(master.data_ptr<float>(), grad.data_ptr<float>(),
                        m.data_ptr<float>(), v.data_ptr<float>(),
                        opt_ptr(shadow), st, (float)lr, (float)b1, (float)b2,
                        (float)eps, zero_grad ? 1 : 0,
                        opt_ptr<float>(extra_zero),
                        extra_zero.has_value() ? extra_zero->numel() : 0,
                        opt_ptr(grad_bf16), (float)grad_scale,
                        opt_ptr<float>(probe_prev),
                        opt_ptr<float>(probe_sumsq),
                        opt_ptr<float>(probe_out), table, T, out, chunks,
                        nchunks, cur_stream());
}

void sgd_step_live(Tensor master, Tensor grad, c10::optional<Tensor> mom,
                   c10::optional<Tensor> shadow, c10::optional<Tensor> step_t,
                   c10::optional<Tensor> lr_table,
                   c10::optional<Tensor> lr_out, double lr, double mu,
                   bool nesterov, bool zero_grad, Tensor live,
                   c10::optional<Tensor> grad_bf16, double grad_scale,
                   c10::optional<Tensor> probe_prev,
                   c10::optional<Tensor> probe_sumsq,
                   c10::optional<Tensor> probe_out) {
  check_f32(master, "master");
  check_probe(probe_prev, probe_sumsq, probe_out);
  TORCH_CHECK(grad.numel() == master.numel()
                  && (!mom.has_value() || mom->numel() == master.numel()),
              "grad / mom must match master's size");
  TORCH_CHECK(!nesterov || (mom.has_value() && mu > 0.0),
              "nesterov needs a momentum buffer and momentum > 0");
  int nchunks = 0;
  const int* chunks = live_table(live, master, &nchunks);
  long T = 0;
  const float* table = sched_table(lr_table, master, &T);
  TORCH_CHECK(table == nullptr || step_t.has_value(),
              "lr_table needs the step_t device counter");
  float* out = sched_scalar(lr_out, master, "lr_out");
  float* st = sched_scalar(step_t, master, "step_t");
  launch_sgd_step_live(master.data_ptr<float>(), grad.data_ptr<float>(),
                       opt_ptr<float>(mom), opt_ptr(shadow), (float)lr,
                       (float)mu, zero_grad ? 1 : 0, opt_ptr(grad_bf16),
                       (float)grad_scale, opt_ptr<float>(probe_prev),
                       opt_ptr<float>(probe_sumsq), opt_ptr<float>(probe_out),
                       st, table, T, out, nesterov ? 1 : 0, chunks, nchunks,
                       cur_stream());
}

void permute_krsc_rsck(Tensor src, Tensor dst, Tensor meta,
                       int64_t max_elem) {
  TORCH_CHECK(meta.scalar_type() == torch::kInt32 && meta.is_cuda());
  launch_permute_krsc_rsck(src.data_ptr(), dst.data_ptr(),
                           meta.data_ptr<int>(), (int)meta.size(0),
                           (int)max_elem, cur_stream());
}

void grad_divergence(Tensor g, Tensor prev, Tensor sumsq, Tensor out,
                     bool skip_first) {
  launch_grad_divergence(g.data_ptr<float>(), prev.data_ptr<float>(),
                         sumsq.data_ptr<float>(), out.data_ptr<float>(),
                         g.numel(), skip_first ? 1 : 0, cur_stream());
}

// uint8 NCHW batch -> normalized bf16 channels_last, one kernel (the
// engines' H2D preprocessing; reference transform (0.5,0.5,0.5) mean/std,
// data_parallel_train.py:44-47).
// Debug/tuning entry: launch the BN-backward reduce directly (variant
// pinned by HZ_BN_V8) for kernel-isolation timing sweeps.
void bn_reduce_bench(Tensor dy, Tensor y, Tensor x, Tensor mean,
                     Tensor invstd, Tensor gamma, Tensor beta, Tensor sdz,
                     Tensor sdzx, int64_t M, int64_t C, int64_t mask) {
  launch_bnact_bwd_reduce(dy.data_ptr(), y.data_ptr(), x.data_ptr(),
                          mean.data_ptr<float>(), invstd.data_ptr<float>(),
                          gamma.data_ptr<float>(), beta.data_ptr<float>(),
                          sdz.data_ptr<float>(), sdzx.data_ptr<float>(), M,
                          (int)C, (int)mask, cur_stream());
}

// Tuning entries for the channel-owner BN kernels: run one forward
// (split-K slabs) or backward BN pair either as the two-kernel path
// (lpr = 0) or as the owner kernel pinned to `lpr` lanes per row.  Return
// the lanes-per-row actually launched (narrowed to fit C and LDS).
int64_t bn_fwd_pair_bench(Tensor ws, c10::optional<Tensor> res, Tensor y,
                          Tensor convout, Tensor stats, Tensor gamma,
                          Tensor beta, Tensor rmean, Tensor rvar,
                          Tensor smean, Tensor sinvstd, int64_t M, int64_t C,
                          int64_t nsplit, int64_t act, int64_t lpr) {
  TORCH_CHECK(ws.numel() >= nsplit * M * C && y.numel() >= M * C &&
                  convout.numel() >= M * C && stats.numel() >= 2 * C,
              "bn_fwd_pair_bench: buffers smaller than nsplit*M*C");
  const void* rp = opt_ptr(res);
  auto st = cur_stream();
  if (lpr == 0) {
    launch_stats_reduce(ws.data_ptr<float>(), stats.data_ptr<float>(), M,
                        (int)C, (int)nsplit, st);
    launch_bn_apply_f32(ws.data_ptr<float>(), rp, y.data_ptr(),
                        convout.data_ptr(), stats.data_ptr<float>(),
                        gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        rmean.data_ptr<float>(), rvar.data_ptr<float>(),
                        smean.data_ptr<float>(), sinvstd.data_ptr<float>(),
                        M, (int)C, 0.1f, 1e-5f, 1, (int)act, (int)nsplit,
                        st);
    return 0;
  }
  int own = bn_owner_fwd_pick(M, (int)C, (int)lpr);
  TORCH_CHECK(own > 0, "owner forward kernel does not take M=", M, " C=", C);
  launch_bn_fwd_owner(ws.data_ptr<float>(), rp, y.data_ptr(),
                      convout.data_ptr(), gamma.data_ptr<float>(),
                      beta.data_ptr<float>(), rmean.data_ptr<float>(),
                      rvar.data_ptr<float>(), smean.data_ptr<float>(),
                      sinvstd.data_ptr<float>(), M, (int)C, 0.1f, 1e-5f,
                      (int)act, (int)nsplit, own, st);
  return own;
}

int64_t bn_bwd_pair_bench(Tensor dy, Tensor y, Tensor x, Tensor mean,
                          Tensor invstd, Tensor gamma, Tensor beta,
                          Tensor sdz, Tensor sdzx, Tensor dconv,
                          c10::optional<Tensor> dres, int64_t M, int64_t C,
                          int64_t mask, int64_t lpr) {
  TORCH_CHECK(dy.numel() >= M * C && y.numel() >= M * C &&
                  x.numel() >= M * C && dconv.numel() >= M * C &&
                  sdz.numel() >= C && sdzx.numel() >= C,
              "bn_bwd_pair_bench: buffers smaller than M*C");
  void* drp = opt_ptr(dres);
  auto st = cur_stream();
  if (lpr == 0) {
    launch_bnact_bwd_reduce(dy.data_ptr(), y.data_ptr(), x.data_ptr(),
                            mean.data_ptr<float>(), invstd.data_ptr<float>(),
                            gamma.data_ptr<float>(), beta.data_ptr<float>(),
                            sdz.data_ptr<float>(), sdzx.data_ptr<float>(), M,
                            (int)C, (int)mask, st);
    launch_bn_bwd_apply(dy.data_ptr(), y.data_ptr(), x.data_ptr(),
                        mean.data_ptr<float>(), invstd.data_ptr<float>(),
                        gamma.data_ptr<float>(), beta.data_ptr<float>(),
                        sdz.data_ptr<float>(), sdzx.data_ptr<float>(),
                        dconv.data_ptr(), drp, M, (int)C, (int)mask, st);
    return 0;
  }
  int own = bn_owner_bwd_pick(M, (int)C, (int)lpr);
  TORCH_CHECK(own > 0, "owner backward kernel does not take M=", M, " C=", C);
  launch_bn_bwd_owner(dy.data_ptr(), y.data_ptr(), x.data_ptr(),
                      mean.data_ptr<float>(), invstd.data_ptr<float>(),
                      gamma.data_ptr<float>(), beta.data_ptr<float>(),
                      sdz.data_ptr<float>(), sdzx.data_ptr<float>(),
                      dconv.data_ptr(), drp, M, (int)C, (int)mask, own, st);
  return own;
}

Tensor normalize_u8(Tensor x, double mean, double std) {
  TORCH_CHECK(x.dim() == 4 && x.dtype() == torch::kUInt8 && x.is_cuda()
                  && x.is_contiguous(),
              "normalize_u8 expects contiguous NCHW uint8 on GPU");
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  auto y = at::empty({N, C, H, W},
                     x.options().dtype(torch::kBFloat16),
                     at::MemoryFormat::ChannelsLast);
  launch_normalize_u8(x.data_ptr(), y.data_ptr(), N * C * H * W, (int)C,
                      H * W, (float)mean, (float)std, cur_stream());
  return y;
}

// normalize_u8 with a per-sample random crop (zero padding `pad`) and
// horizontal flip folded in.  `state` = int64 {key, step}; the op advances
// the step on the device (graph-replay safe).  `params` (int32 [N],
// dy | dx<<8 | flip<<16) overrides the RNG and leaves `state` untouched.
Tensor augment_normalize_u8(Tensor x, Tensor state, double mean, double std,
                            int64_t pad, bool flip,
                            c10::optional<Tensor> params) {
  TORCH_CHECK(x.dim() == 4 && x.dtype() == torch::kUInt8 && x.is_cuda()
                  && x.is_contiguous(),
              "augment_normalize_u8 expects contiguous NCHW uint8 on GPU");
  TORCH_CHECK(pad >= 0 && pad <= 127,
              "augment_normalize_u8: pad must be in [0, 127], got ", pad);
  TORCH_CHECK(state.is_cuda() && state.dtype() == torch::kInt64
                  && state.is_contiguous() && state.numel() >= 2
                  && state.device() == x.device(),
              "augment_normalize_u8: state must be a contiguous int64 GPU "
              "tensor with >= 2 elements (key, step)");
  const long N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(N * C * H * W < (1L << 31),
              "augment_normalize_u8: batch too large for 32-bit indexing");
  const int* pp = nullptr;
  if (params.has_value()) {
    const Tensor& p = *params;
    TORCH_CHECK(p.is_cuda() && p.dtype() == torch::kInt32
                    && p.is_contiguous() && p.numel() == N
                    && p.device() == x.device(),
                "augment_normalize_u8: params must be a contiguous int32 GPU "
                "tensor with N = ", N, " elements");
    pp = p.data_ptr<int>();
  }
  auto y = at::empty({N, C, H, W},
                     x.options().dtype(torch::kBFloat16),
                     at::MemoryFormat::ChannelsLast);
  launch_augment_normalize_u8(x.data_ptr(), y.data_ptr(), state.data_ptr(),
                              pp, N, (int)C, (int)H, (int)W, (int)pad,
                              flip ? 1 : 0, (float)mean, (float)std,
                              cur_stream());
  return y;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("conv_bn_act_fwd", &conv_bn_act_fwd);
  m.def("conv_bn_act_bwd", &conv_bn_act_bwd);
  m.def("dw_conv_bn_fwd", &dw_conv_bn_fwd);
  m.def("dw_conv_bn_bwd", &dw_conv_bn_bwd);
  m.def("maxpool_fwd", &maxpool_fwd);
  m.def("maxpool_bwd", &maxpool_bwd);
  m.def("avgpool_fwd", &avgpool_fwd);
  m.def("avgpool_bwd", &avgpool_bwd);
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_bwd", &linear_bwd);
  m.def("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd);
  m.def("gemm_bf16", &gemm_bf16);
  m.def("adam_step", &adam_step);
  m.def("sgd_step", &sgd_step);
  m.def("cross_entropy_ls_fwd_bwd", &cross_entropy_ls_fwd_bwd);
  m.def("adam_step_sched", &adam_step_sched, py::arg("master"),
        py::arg("grad"), py::arg("m"), py::arg("v"), py::arg("shadow"),
        py::arg("step_t"), py::arg("lr_table"), py::arg("lr_out"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("wd"), py::arg("decoupled"), py::arg("zero_grad"),
        py::arg("extra_zero") = py::none(), py::arg("grad_bf16") = py::none(),
        py::arg("grad_scale") = 1.0, py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("sgd_step_sched", &sgd_step_sched, py::arg("master"),
        py::arg("grad"), py::arg("mom"), py::arg("shadow"), py::arg("step_t"),
        py::arg("lr_table"), py::arg("lr_out"), py::arg("lr"), py::arg("mu"),
        py::arg("wd"), py::arg("nesterov"), py::arg("zero_grad"),
        py::arg("grad_bf16") = py::none(), py::arg("grad_scale") = 1.0,
        py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("seg_norms", &seg_norms, py::arg("master"), py::arg("grad"),
        py::arg("chunks"), py::arg("seg_meta"), py::arg("partials"),
        py::arg("seg_norms"), py::arg("seg_mul"), py::arg("norm_out"),
        py::arg("wd"), py::arg("max_norm"), py::arg("lars"), py::arg("eta"),
        py::arg("grad_bf16") = py::none(), py::arg("grad_scale") = 1.0);
  m.def("adam_step_seg", &adam_step_seg, py::arg("master"), py::arg("grad"),
        py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("step_t"),
        py::arg("lr_table"), py::arg("lr_out"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("decoupled"),
        py::arg("zero_grad"), py::arg("chunks"), py::arg("seg_mul"),
        py::arg("extra_zero") = py::none(), py::arg("grad_bf16") = py::none(),
        py::arg("grad_scale") = 1.0, py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("sgd_step_seg", &sgd_step_seg, py::arg("master"), py::arg("grad"),
        py::arg("mom"), py::arg("shadow"), py::arg("step_t"),
        py::arg("lr_table"), py::arg("lr_out"), py::arg("lr"), py::arg("mu"),
        py::arg("nesterov"), py::arg("zero_grad"), py::arg("chunks"),
        py::arg("seg_mul"), py::arg("grad_bf16") = py::none(),
        py::arg("grad_scale") = 1.0, py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("adam_step_live", &adam_step_live, py::arg("master"),
        py::arg("grad"), py::arg("m"), py::arg("v"), py::arg("shadow"),
        py::arg("step_t"), py::arg("lr_table"), py::arg("lr_out"),
        py::arg("lr"), py::arg("b1"), py::arg("b2"), py::arg("eps"),
        py::arg("zero_grad"), py::arg("live"),
        py::arg("extra_zero") = py::none(), py::arg("grad_bf16") = py::none(),
        py::arg("grad_scale") = 1.0, py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("sgd_step_live", &sgd_step_live, py::arg("master"), py::arg("grad"),
        py::arg("mom"), py::arg("shadow"), py::arg("step_t"),
        py::arg("lr_table"), py::arg("lr_out"), py::arg("lr"), py::arg("mu"),
        py::arg("nesterov"), py::arg("zero_grad"), py::arg("live"),
        py::arg("grad_bf16") = py::none(), py::arg("grad_scale") = 1.0,
        py::arg("probe_prev") = py::none(),
        py::arg("probe_sumsq") = py::none(),
        py::arg("probe_out") = py::none());
  m.def("tap_window_registry", &tap_window_registry);
  m.def("tap_window_version", &tap_window_version);
  m.def("tap_window_reset", &tap_window_reset, py::arg("lo") = 0,
        py::arg("hi") = 0);
  m.def("set_opt_skip_dead", &set_opt_skip_dead);
  m.def("opt_skip_dead_enabled", &opt_skip_dead_enabled);
  m.def("permute_krsc_rsck", &permute_krsc_rsck);
  m.def("grad_divergence", &grad_divergence);
  m.def("normalize_u8", &normalize_u8);
  m.def("augment_normalize_u8", &augment_normalize_u8, py::arg("x"),
        py::arg("state"), py::arg("mean"), py::arg("std"), py::arg("pad"),
        py::arg("flip"), py::arg("params") = py::none());
  m.def("bn_reduce_bench", &bn_reduce_bench);
  m.def("bn_fwd_pair_bench", &bn_fwd_pair_bench);
  m.def("bn_bwd_pair_bench", &bn_bwd_pair_bench);
  m.def("set_bn_owner", &set_bn_owner);
  m.def("bn_owner_enabled", &bn_owner_enabled);
  m.def("bn_owner_launches", &bn_owner_launches);
  m.def("set_deterministic", &set_deterministic);
  m.def("deterministic_enabled", &deterministic_enabled);
  m.def("set_wgrad_defer", &set_wgrad_defer);
  m.def("wgrad_defer_enabled", &wgrad_defer_enabled);
  m.def("wgrad_pending", &wgrad_pending);
  m.def("flush_wgrad", &flush_wgrad);
  m.def("flush_wgrad_range", &flush_wgrad_range);
  m.def("wgrad_only", &wgrad_only);
  m.def("conv_dgrad_only", &conv_dgrad_only);
  m.def("set_dgrad_krsc", &set_dgrad_krsc);
  m.def("dgrad_krsc_enabled", &dgrad_krsc_enabled);
  m.def("set_wgrad_tr", &set_wgrad_tr);
  m.def("wgrad_tr_enabled", &wgrad_tr_enabled);
  m.def("set_tap_clip", &set_tap_clip);
  m.def("tap_clip_enabled", &tap_clip_enabled);
  m.def("conv_tap_window", &conv_tap_window);
}
