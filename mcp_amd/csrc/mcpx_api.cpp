// mcpx_api.cpp — implementation of the C ABI declared in include/mcpx.h.
//
// Host side of the drop-in boundary for src/solver.jl:35-122: argument checks
// (the reference's own ArgumentError / @assert sites, src/AutoDiff.jl:19-23,
// src/mcp.jl:191), the per-call constant tables the reference computes inline
// (line-search step sizes src/solver.jl:127-138, ϵ-schedule factors
// src/solver.jl:111-113), device selection, batch sharding over GPUs and
// stream-ordered launches.  Reentrant: no global mutable state apart from the
// thread-local error string.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcpx.h"
#include "dev_pool.hpp"
#include "ipm_kernel.h"
#include "ipm_wg.h"
#include "sens_kernel.h"
#include "wg_layout.h"

// Fields of the record mcpx_nl_meta that a generated module exports (defined, with the
// kernel mask's bits, at the end of csrc/ipm_nl_kernel.hpp).
enum NLMeta {
  kMetaLayout = 0,   // layout version: kNLLayout
  kMetaN = 1,
  kMetaM = 2,
  kMetaP = 3,        // θ dimension
  kMetaKernels = 5,  // kernel mask
  kMetaBlock = 6,    // doubles of the generated Jacobian blocks (MCPX_NL_SIZE)
  kMetaBandWs = 9,   // the band kernel's workspace doubles per slot
};
constexpr int32_t kNLLayout = 4;

// A generated nonlinear module (MCPX_FAMILY_NONLINEAR, include/mcpx.h): the
// code object image, its metadata record and the per-device loaded modules.
struct mcpx_module {
  std::vector<char> image;
  int32_t meta[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // indexed by NLMeta
  std::mutex mu;
  std::map<int, hipModule_t> loaded;  // device → module, loaded on first use
  bool has(int bit) const { return (meta[kMetaKernels] >> bit) & 1; }  // a bit of the kernel mask
};

namespace {

namespace wg = mcpx::wg;

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(MCPX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));            \
  } while (0)

int check_device(int dev) {
  static std::atomic<uint64_t> verified{0};  // devices already found to be gfx950 (bit per ordinal < 64)
  if (dev >= 0 && dev < 64 && ((verified.load(std::memory_order_relaxed) >> dev) & 1)) return MCPX_OK;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MCPX_ENODEV, "device %d is %s; this build targets gfx950 (MI355X) only", dev,
                prop.gcnArchName);
  if (dev >= 0 && dev < 64) verified.fetch_or(uint64_t(1) << dev, std::memory_order_relaxed);
  return MCPX_OK;
}

// The current device of a device-buffer call: MCPX_ENODEV when none is visible.
int current_device(int* dev) {
  const hipError_t e = hipGetDevice(dev);
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return fail(MCPX_ENODEV, "no HIP device visible");
  HIP_TRY(e);
  return check_device(*dev);
}

// MCPX_GENERIC_KERNELS=1 disables the compile-time-(n, m) kernels (A/B switch).
bool specialized_enabled() {
  const char* e = std::getenv("MCPX_GENERIC_KERNELS");
  return !(e && e[0] == '1');
}

// Register-row width of the runtime-(n, m) kernels: smallest compiled width ≥ N.
int pick_nmax(int N) {
  for (int w : {8, 16, 24, 32, 48, 64})
    if (N <= w) return w;
  return -1;
}

// Smallest workgroup-kernel vector-dimension bucket ≥ N (QP / affine), or -1.
int pick_wg_bucket(int N) {
  for (int w : wg::kDimBuckets)
    if (N <= w) return w;
  return -1;
}

// What a call does with a generated module, for the two messages of check_desc that say so.
struct Wording {
  const char *does, *goes, *entry;
};
constexpr Wording kSolveWords = {"solves", "runs", "mcpx_solve_batch_module*"};
constexpr Wording kSensWords = {"differentiates", "is differentiated", "mcpx_vjp_batch_module / mcpx_jvp_batch_module"};

// The descriptor checks shared by the solves and the sensitivities; *pd: the θ dimension
// (of the family, or of the generated module `mod`); `split` (mcpx_solve_batch_shared*): of the
// family's per-instance block, the stride desc->theta_ld then counts.
int check_desc(const mcpx_desc* d, const mcpx_module* mod, int64_t* pd, const Wording& w, bool split = false) {
  if (mod) {  // a generated nonlinear module: θ dimension and sizes from its metadata
    if (d->family != MCPX_FAMILY_NONLINEAR)
      return fail(MCPX_EINVAL, "a generated module %s family MCPX_FAMILY_NONLINEAR (got %d)", w.does, d->family);
    if (d->n != mod->meta[kMetaN] || d->m != mod->meta[kMetaM])
      return fail(MCPX_EINVAL, "desc (n=%d, m=%d) does not match the module (n=%d, m=%d)", d->n, d->m,
                  mod->meta[kMetaN], mod->meta[kMetaM]);
    *pd = mod->meta[kMetaP];
  } else {
    if (d->family == MCPX_FAMILY_NONLINEAR)
      return fail(MCPX_EINVAL, "family MCPX_FAMILY_NONLINEAR %s through its generated module (%s)", w.goes, w.entry);
    *pd = split ? mcpx_theta_var_dim(d->family, d->n, d->m) : mcpx_theta_dim(d->family, d->n, d->m);
  }
  if (*pd < 0) return fail(MCPX_EINVAL, "bad family %d or negative dimensions (n=%d, m=%d)", d->family, d->n, d->m);
  if (d->n + d->m < 1) return fail(MCPX_EINVAL, "empty problem (n = m = 0)");
  if (d->batch < 0) return fail(MCPX_EINVAL, "negative batch");
  if (d->theta_ld < *pd) return fail(MCPX_EINVAL, "theta_ld %lld < parameter dimension %lld", (long long)d->theta_ld, (long long)*pd);
  return MCPX_OK;
}

// How a solve runs: the one-wave kernels (`nmax`: their row width), the workgroup-per-instance
// kernels (wg; ipm_wg_impl.hpp, `nmax`: their dimension bucket), or a generated module's
// (`mod`) one-wave, workgroup, multi-wave (mw) or band kernel.
struct SolvePlan {
  int nmax = 0;
  bool wg = false, mw = false, band = false;
  mcpx_module* mod = nullptr;
};

// Validates desc/params; fills the scalar part + tables of the kernel args and the plan.
// `split`: a shared-matrix call (desc->theta_ld is the stride of the per-instance block).
int prepare(const mcpx_desc* d, const mcpx_params* p, mcpx::KernelArgs* a, SolvePlan* plan, mcpx_module* mod,
            bool split = false) {
  *plan = SolvePlan{};
  plan->mod = mod;
  if (!d || !p) return fail(MCPX_EINVAL, "desc and params must be non-NULL");
  int64_t pd;
  if (const int rc = check_desc(d, mod, &pd, kSolveWords, split)) return rc;
  const int ls = p->linear_solver;
  if (ls != MCPX_LINSOLVE_REDUCED && ls != MCPX_LINSOLVE_DENSE && ls != MCPX_LINSOLVE_SCHUR)
    return fail(MCPX_EINVAL, "unknown linear_solver %d", ls);
  if (p->kernel != MCPX_KERNEL_AUTO && p->kernel != MCPX_KERNEL_WAVE && p->kernel != MCPX_KERNEL_WORKGROUP &&
      p->kernel != MCPX_KERNEL_MULTIWAVE && p->kernel != MCPX_KERNEL_BAND)
    return fail(MCPX_EINVAL, "unknown kernel selector %d", p->kernel);
  bool wave_ok, wg_ok;
  if (mod) {
    wave_ok = mod->has(ls);
    wg_ok = mod->has(3 + ls);
    const bool mw_ok = ls == MCPX_LINSOLVE_SCHUR && mod->has(MCPX_MODULE_SCHUR_MW);
    if (p->kernel == MCPX_KERNEL_MULTIWAVE && !mw_ok)
      return fail(MCPX_EUNSUPPORTED, "the generated module has no multi-wave kernel for linear_solver=%d", ls);
    plan->mw = mw_ok && p->kernel == MCPX_KERNEL_MULTIWAVE;  // measured slower than one wave: opt-in
    // the band kernel (ipm_nl_band.hpp): forced, or AUTO when the module prefers it or has no
    // one-wave SCHUR kernel (oracle/ipm_oracle.c picks lu_band_solve by the same rule)
    const bool band_ok = ls == MCPX_LINSOLVE_SCHUR && mod->has(MCPX_MODULE_BAND);
    const bool band_auto = band_ok && mod->has(MCPX_MODULE_BAND_AUTO);
    if (p->kernel == MCPX_KERNEL_BAND && !band_ok)
      return fail(MCPX_EUNSUPPORTED, "the generated module has no band kernel for linear_solver=%d", ls);
    plan->band = p->kernel == MCPX_KERNEL_BAND || (p->kernel == MCPX_KERNEL_AUTO && band_ok && (band_auto || !wave_ok));
  } else {
    if (p->kernel == MCPX_KERNEL_MULTIWAVE)
      return fail(MCPX_EUNSUPPORTED, "MCPX_KERNEL_MULTIWAVE is a generated module's SCHUR kernel");
    if (p->kernel == MCPX_KERNEL_BAND)
      return fail(MCPX_EUNSUPPORTED, "MCPX_KERNEL_BAND is a generated module's SCHUR kernel");
    // (affine family, SCHUR: the S block of θ (∂H/∂y) is read, and a nonzero or NaN entry ends the
    // instance with MCPX_FAIL_INPUT, include/mcpx.h)
    const int N = ls == MCPX_LINSOLVE_DENSE ? d->n + 2 * d->m : (ls == MCPX_LINSOLVE_REDUCED ? d->n + d->m : d->n);
    const int lanes = ls == MCPX_LINSOLVE_DENSE ? d->n + 2 * d->m : d->n + d->m;  // one wave: one lane per row
    wave_ok = pick_nmax(N) > 0 && lanes <= MCPX_MAX_KKT_DIM;
    // workgroup kernels: REDUCED / DENSE, and SCHUR for the QP family up to n = 128 (gj_vr.hpp)
    wg_ok = (ls != MCPX_LINSOLVE_SCHUR || (d->family == MCPX_FAMILY_QP && d->n <= wg::kGjMax)) &&
            d->n + 2 * d->m <= MCPX_MAX_WG_KKT_DIM;
    plan->nmax = wave_ok && p->kernel != MCPX_KERNEL_WORKGROUP ? pick_nmax(N) : pick_wg_bucket(d->n + 2 * d->m);
  }
  if (p->kernel == MCPX_KERNEL_WAVE) wg_ok = false;
  if (p->kernel == MCPX_KERNEL_WORKGROUP) wave_ok = false;
  if (plan->mw || plan->band) wave_ok = true;
  if (!wave_ok && !wg_ok) {
    if (mod)
      return fail(MCPX_EUNSUPPORTED, "the generated module has no %s kernel for linear_solver=%d (n=%d m=%d)",
                  p->kernel == MCPX_KERNEL_WAVE ? "one-wave" : (p->kernel == MCPX_KERNEL_WORKGROUP ? "workgroup" : ""),
                  ls, d->n, d->m);
    return fail(MCPX_EUNSUPPORTED, "problem size n=%d m=%d, linear_solver=%d exceeds the kernels (one wave: "
                "reduced/schur n+m <= %d, dense n+2m <= %d; workgroup: reduced/dense n+2m <= %d, "
                "schur: QP family, n <= %d)",
                d->n, d->m, ls, MCPX_MAX_KKT_DIM, MCPX_MAX_KKT_DIM, MCPX_MAX_WG_KKT_DIM, wg::kGjMax);
  }
  plan->wg = !wave_ok;
  if (!(p->tol > 0) || !(p->min_stepsize > 0) || !(p->decay > 0 && p->decay < 1) || std::isnan(p->tau) ||
      std::isnan(p->tightening_rate) || std::isnan(p->loosening_rate) || p->max_inner_iters < 1 ||
      p->max_outer_iters < 1)
    return fail(MCPX_EINVAL, "invalid solver parameters (tol>0, min_stepsize>0, 0<decay<1, iteration limits >= 1)");
  if (p->max_inner_iters > MCPX_MAX_INNER_ITERS)
    return fail(MCPX_EUNSUPPORTED, "max_inner_iters %d > %d", p->max_inner_iters, MCPX_MAX_INNER_ITERS);
  std::memset(a, 0, sizeof *a);
  a->n = d->n;
  a->m = d->m;
  a->solver = ls;
  a->family = d->family;
  a->theta_ld = d->theta_ld;
  a->max_inner = p->max_inner_iters;
  a->max_outer = p->max_outer_iters;
  a->tol = p->tol;
  a->decay = p->decay;
  a->c_tau = 1.0 - p->tau;  // src/solver.jl:129 (1 - τ)
  // src/solver.jl:128-135: trials α = 1, decay, decay², … until α < min_stepsize
  double al = 1.0;
  int e = 0;
  for (;;) {
    if (e >= MCPX_MAX_LS_TRIALS) return fail(MCPX_EUNSUPPORTED, "min_stepsize/decay need more than %d line-search trials", MCPX_MAX_LS_TRIALS);
    if (al < p->min_stepsize) break;
    al *= p->decay;
    ++e;
  }
  a->n_trials = e + 1;
  for (int k = 0; k <= p->max_inner_iters; ++k) {  // src/solver.jl:111-113
    a->tight[k] = 1.0 - std::exp(-p->tightening_rate * (double)k);
    a->loose[k] = 1.0 + std::exp(-p->loosening_rate * (double)k);
  }
  return MCPX_OK;
}

// ---- generated nonlinear modules ---------------------------------------------
const char* const kNLKernel[3] = {"mcpx_nl_solve_reduced", "mcpx_nl_solve_dense", "mcpx_nl_solve_schur"};

// `mod` on device `dev` (the current device), loaded on first use.
int module_on(mcpx_module* mod, int dev, hipModule_t* hm) {
  std::lock_guard<std::mutex> lock(mod->mu);
  auto it = mod->loaded.find(dev);
  if (it != mod->loaded.end()) {
    *hm = it->second;
    return MCPX_OK;
  }
  HIP_TRY(hipModuleLoadData(hm, mod->image.data()));
  mod->loaded[dev] = *hm;
  return MCPX_OK;
}

// The module's kernel `name` (`shown` in the message when it has none) on the current
// device, *dev.
int module_function(mcpx_module* mod, const char* name, const char* shown, hipFunction_t* f, int* dev) {
  HIP_TRY(hipGetDevice(dev));
  hipModule_t hm;
  const int rc = module_on(mod, *dev, &hm);
  if (rc) return rc;
  if (hipModuleGetFunction(f, hm, name) != hipSuccess)
    return fail(MCPX_EUNSUPPORTED, "the generated module has no %s kernel", shown);
  return MCPX_OK;
}

// The module's solve kernel for linear solver `solver`: one-wave (suffix ""), workgroup
// ("_wg") or multi-wave ("_mw").
int nl_function(mcpx_module* mod, int solver, const char* suffix, hipFunction_t* f) {
  const std::string name = std::string(kNLKernel[solver]) + suffix;
  int dev = 0;
  return module_function(mod, name.c_str(), name.c_str(), f, &dev);
}

hipError_t launch_module(hipFunction_t f, int64_t grid, unsigned threads, void* args, hipStream_t st) {
  void* params[] = {args};
  return hipModuleLaunchKernel(f, (unsigned)grid, 1, 1, threads, 1, 1, 0, st, params, nullptr);
}

// Picks the kernel: a compile-time-(n, m) specialisation when one exists (and
// MCPX_GENERIC_KERNELS is not set), else the runtime-(n, m) kernel for nmax.
hipError_t launch(int nmax, const mcpx::KernelArgs& a, int64_t nb, hipStream_t st) {
  if (specialized_enabled()) {
    const hipError_t e = mcpx::launch_ipm_spec(a.family, a.solver, a.n, a.m, a, nb, st);
    if (e != hipErrorNotFound) return e;
  }
  const bool qp = a.family == MCPX_FAMILY_QP;
  switch (a.solver) {
    case MCPX_LINSOLVE_REDUCED:
      return qp ? mcpx::launch_ipm_red_qp(nmax, a, nb, st) : mcpx::launch_ipm_red_aff(nmax, a, nb, st);
    case MCPX_LINSOLVE_DENSE:
      return qp ? mcpx::launch_ipm_dense_qp(nmax, a, nb, st) : mcpx::launch_ipm_dense_aff(nmax, a, nb, st);
    default:
      return qp ? mcpx::launch_ipm_schur_qp(nmax, a, nb, st) : mcpx::launch_ipm_schur_aff(nmax, a, nb, st);
  }
}

// uint64 words of one instance's active-set mask: ⌈m/64⌉, at least 1 (include/mcpx.h)
inline int64_t mask_words(int m) { return m > 64 ? (m + 63) / 64 : 1; }

// Doubles a copy of `nb` strided instances may touch, `own` doubles each at stride `ld` >= own:
// the last instance ends with its own doubles, not with the stride — the caller's buffer may
// end there (include/mcpx.h: the ld − own doubles after an instance are never read).  Every
// host-side copy of a strided θ block sizes itself here.
inline size_t strided_span(int64_t nb, int64_t ld, int64_t own) {
  return nb > 0 ? (size_t)((nb - 1) * ld + own) : 0;
}

// ---- grouped shared-matrix batches (mcpx_*_batch_grouped*) -------------------------------------

// What a grouped call derives from its host metadata, once, before any launch.
struct GroupTable {
  int64_t G = 0;
  std::vector<int32_t> map;              // [B]: instance → group, the kernels' lookup
  std::vector<double> packed;            // host entries, padded blocks: the G blocks at stride shared_dim
  std::vector<mcpx::GroupChunk> chunks;  // reduce entries: chunks of MCPX_REDUCE_CHUNK counted from each off[g]
  std::vector<int64_t> cbase;            // reduce entries, [G + 1]: group g owns chunks [cbase[g], cbase[g + 1])
};

// The argument checks of the grouped entries after the descriptor's (ds: mcpx_theta_shared_dim).
int check_groups(const mcpx_desc* d, const double* shared, int64_t shared_ld, int32_t G, const int64_t* off,
                 int64_t ds) {
  if (G < 0) return fail(MCPX_EINVAL, "negative num_groups");
  if (shared_ld < ds) return fail(MCPX_EINVAL, "shared_ld %lld < shared dimension %lld", (long long)shared_ld, (long long)ds);
  if (d->batch > 0 && (G == 0 || !shared || !off))
    return fail(MCPX_EINVAL, "a non-empty grouped batch needs num_groups >= 1, theta_shared and group_offsets");
  if (off) {
    if (off[0] != 0 || off[G] != d->batch)
      return fail(MCPX_EINVAL, "group_offsets must run from 0 to batch (%lld): got %lld .. %lld", (long long)d->batch,
                  (long long)off[0], (long long)off[G]);
    for (int32_t g = 0; g < G; ++g)
      if (off[g + 1] < off[g]) return fail(MCPX_EINVAL, "group_offsets decrease at group %d", g);
  }
  return MCPX_OK;
}

// The tables of a checked, non-empty grouped call.  `pack` (host entries): the blocks for upload.
void build_groups(const mcpx_desc* d, const double* shared, int64_t shared_ld, int32_t G, const int64_t* off,
                  int64_t ds, bool pack, bool reduce, GroupTable* t) {
  t->G = G;
  t->map.resize((size_t)d->batch);
  for (int32_t g = 0; g < G; ++g) std::fill(t->map.begin() + off[g], t->map.begin() + off[g + 1], g);
  if (pack && shared_ld != ds) {
    t->packed.resize((size_t)(G * ds));
    for (int32_t g = 0; g < G; ++g) std::copy(shared + g * shared_ld, shared + g * shared_ld + ds, t->packed.begin() + g * ds);
  }
  if (!reduce) return;
  t->cbase.assign((size_t)G + 1, 0);
  for (int32_t g = 0; g < G; ++g) {
    for (int64_t b = off[g]; b < off[g + 1]; b += MCPX_REDUCE_CHUNK)
      t->chunks.push_back(mcpx::GroupChunk{b, (int32_t)std::min<int64_t>(MCPX_REDUCE_CHUNK, off[g + 1] - b), g});
    t->cbase[(size_t)g + 1] = (int64_t)t->chunks.size();
  }
}

// The tables of a device-buffer call on the device: one block of the cache, filled on `st` from a
// pinned staging buffer of the library's (the caller's offsets are not read after the call returns).
struct DevGroups {
  AsyncBuf<char> blk;
  const int32_t* map = nullptr;
  const mcpx::GroupChunk* chunks = nullptr;
  const int64_t* cbase = nullptr;
  hipError_t upload(const GroupTable& t, hipStream_t st) {
    const size_t nm = (t.map.size() * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t nc = t.chunks.size() * sizeof(mcpx::GroupChunk), nb = t.cbase.size() * sizeof(int64_t);
    const size_t bytes = nm + nc + nb;
    hipError_t e = blk.alloc(bytes, st);
    if (e != hipSuccess) return e;
    void* h = nullptr;
    if ((e = stage_acquire(bytes, &h)) != hipSuccess) return e;
    std::memcpy(h, t.map.data(), t.map.size() * sizeof(int32_t));
    if (nc) std::memcpy((char*)h + nm, t.chunks.data(), nc);
    if (nb) std::memcpy((char*)h + nm + nc, t.cbase.data(), nb);
    e = hipMemcpyAsync(blk.p, h, bytes, hipMemcpyHostToDevice, st);
    stage_release(h, st);
    map = (const int32_t*)blk.p;
    chunks = (const mcpx::GroupChunk*)(blk.p + nm);
    cbase = (const int64_t*)(blk.p + nm + nc);
    return e;
  }
};

// Per-instance pointers of chunk [b0, b0 + nb) into the kernel args.
void set_chunk(mcpx::KernelArgs& a, const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
               const double* s0, const mcpx_out* o, int64_t b0) {
  const int n = d->n, m = d->m;
  a.theta = theta + b0 * d->theta_ld;
  a.x0 = x0 ? x0 + b0 * n : nullptr;
  a.y0 = y0 ? y0 + b0 * m : nullptr;
  a.s0 = s0 ? s0 + b0 * m : nullptr;
  a.x = o->x + b0 * n;
  a.y = o->y + b0 * m;
  a.s = o->s + b0 * m;
  a.kkt_error = o->kkt_error + b0;
  a.eps = o->eps + b0;
  a.outer_iters = o->outer_iters + b0;
  a.status = o->status + b0;
  a.newton_iters = o->newton_iters ? o->newton_iters + b0 : nullptr;
  a.active_mask = o->active_mask ? o->active_mask + b0 * mask_words(m) : nullptr;
  a.alpha_trace = (o->alpha_trace && o->trace_len > 0) ? o->alpha_trace + b0 * (int64_t)o->trace_len * 2 : nullptr;
  a.trace_len = o->alpha_trace ? o->trace_len : 0;
  a.fail_reason = o->fail_reason ? o->fail_reason + b0 : nullptr;
}

// A kernel of the persistent-grid launches: a generated module's function or a host symbol.
struct GridKernel {
  hipFunction_t f = nullptr;
  const void* sym = nullptr;
  int threads = wg::kThreads;
};

// The persistent-grid launch of the workgroup-per-instance kernels and the band kernel: a
// grid of the resident workgroups (occupancy × CUs of device `dev`; -1: the current one,
// asked for here) pulls instances from an atomic counter; each workgroup slot owns
// w.slot_stride doubles of workspace in HBM (at most `cap_bytes` in all, 0: no cap), allocated
// stream-ordered for this call with the counter behind it.  `w` (WgArgs / WgSensArgs) gets
// the workspace, the counter and each chunk's batch; launch(b0, grid) fills the rest for
// the chunk that starts at instance b0 and launches `grid` workgroups.
template <class W, class Launch>
int launch_persistent(const GridKernel& k, int dev, int64_t batch, W& w, int64_t cap_bytes, hipStream_t st,
                      const char* what, Launch&& launch) {
  int per_cu = 0, cus = 0;
  if (k.f)
    HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.f, k.threads, 0));
  else
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.sym, k.threads, 0));
  if (dev < 0) HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const int64_t slots = (int64_t)std::max(per_cu, 1) * std::max(cus, 1);
  const int64_t grid_max = wg::grid_size(slots, batch, w.slot_stride, cap_bytes);
  HIP_TRY(dev_alloc((void**)&w.work, sizeof(double) * (size_t)(grid_max * w.slot_stride) + 256, st));
  w.counter = (int32_t*)(w.work + grid_max * w.slot_stride);
  int rc = MCPX_OK;
  for (int64_t b0 = 0; b0 < batch && rc == MCPX_OK; b0 += wg::kChunk) {
    w.batch = std::min(wg::kChunk, batch - b0);
    hipError_t e = hipMemsetAsync(w.counter, 0, sizeof(int32_t), st);
    if (e == hipSuccess) e = launch(b0, (int)std::min(grid_max, w.batch));
    if (e != hipSuccess) rc = fail(MCPX_EHIP, "%s launch failed: %s", what, hipGetErrorString(e));
  }
  dev_release(w.work, st);
  return rc;
}

// Workgroup-per-instance solve (ipm_wg_impl.hpp): the slot holds [K | rhs] row-major, and
// for a generated module its Jacobian blocks (wg_layout.h).
int launch_wg(const mcpx_desc* d, const double* theta, const double* x0, const double* y0, const double* s0,
              const mcpx_out* o, const mcpx::KernelArgs& a, const SolvePlan& plan, hipStream_t st) {
  const int ls = a.solver, nv = plan.nmax, ns = wg::system_rows(ls, d->n, d->m);
  GridKernel k;
  if (plan.mod) {
    const int rc = nl_function(plan.mod, ls, "_wg", &k.f);
    if (rc) return rc;
  } else {
    k.sym = mcpx::ipm_wg_kernel(a.family, ls, nv, ns);
    if (!k.sym) return fail(MCPX_EUNSUPPORTED, "no workgroup kernel for family %d, linear_solver %d, dim %d", a.family, ls, nv);
  }
  wg::WgArgs w = wg::solve_layout(ls, d->n, d->m, plan.mod ? plan.mod->meta[kMetaBlock] : 0);
  return launch_persistent(k, -1, d->batch, w, 0, st, "workgroup solver", [&](int64_t b0, int grid) {
    w.k = a;
    set_chunk(w.k, d, theta, x0, y0, s0, o, b0);
    return plan.mod ? launch_module(k.f, grid, k.threads, &w, st)
                    : mcpx::launch_ipm_wg(a.family, ls, nv, ns, w, grid, st);
  });
}

// The band SCHUR kernel of a generated module (ipm_nl_band.hpp): one wave per resident slot
// on the work queue of the workgroup kernels; the slot is the kernel's own workspace (its U
// rows when they exceed its VGPR budget, else none: LDS and VGPRs only).
int launch_band(const mcpx_desc* d, const double* theta, const double* x0, const double* y0, const double* s0,
                const mcpx_out* o, const mcpx::KernelArgs& a, const SolvePlan& plan, hipStream_t st) {
  GridKernel k;
  k.threads = 64;
  int dev = 0;
  const int rc = module_function(plan.mod, "mcpx_nl_solve_band", "band", &k.f, &dev);
  if (rc) return rc;
  wg::WgArgs w{};
  w.slot_stride = wg::align(plan.mod->meta[kMetaBandWs]);
  return launch_persistent(k, dev, d->batch, w, 0, st, "band solver", [&](int64_t b0, int grid) {
    w.k = a;
    set_chunk(w.k, d, theta, x0, y0, s0, o, b0);
    return launch_module(k.f, grid, k.threads, &w, st);
  });
}

int launch_chunks(const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
                  const double* s0, const mcpx_out* o, mcpx::KernelArgs a, const SolvePlan& plan, hipStream_t st) {
  if (plan.band) return launch_band(d, theta, x0, y0, s0, o, a, plan, st);
  if (plan.wg) return launch_wg(d, theta, x0, y0, s0, o, a, plan, st);
  hipFunction_t nlf = nullptr;  // generated module: its kernel, launched by hipModuleLaunchKernel
  if (plan.mod) {
    const int rc = nl_function(plan.mod, a.solver, plan.mw ? "_mw" : "", &nlf);
    if (rc) return rc;
  }
  const unsigned threads = plan.mw ? 256 : 64;  // the multi-wave SCHUR kernel: 4 waves per instance
  for (int64_t b0 = 0; b0 < d->batch; b0 += wg::kChunk) {
    const int64_t nb = std::min(wg::kChunk, d->batch - b0);
    set_chunk(a, d, theta, x0, y0, s0, o, b0);
    if (plan.mod)
      HIP_TRY(launch_module(nlf, nb, threads, &a, st));
    else
      HIP_TRY(launch(plan.nmax, a, nb, st));
  }
  return MCPX_OK;
}

// The outputs of the instances from b0 on (the host layout of set_chunk's device pointers).
mcpx_out out_at(const mcpx_out* o, int n, int m, int64_t b0) {
  mcpx_out r = *o;
  r.x = o->x + b0 * n;
  r.y = o->y + b0 * m;
  r.s = o->s + b0 * m;
  r.kkt_error = o->kkt_error + b0;
  r.eps = o->eps + b0;
  r.outer_iters = o->outer_iters + b0;
  r.status = o->status + b0;
  r.newton_iters = o->newton_iters ? o->newton_iters + b0 : nullptr;
  r.active_mask = o->active_mask ? o->active_mask + b0 * mask_words(m) : nullptr;
  r.alpha_trace = o->alpha_trace ? o->alpha_trace + b0 * (int64_t)o->trace_len * 2 : nullptr;
  r.fail_reason = o->fail_reason ? o->fail_reason + b0 : nullptr;
  return r;
}

// Bytes of the θ′ expansion block of a shared-matrix call (below): MCPX_EXPAND_MB MiB (A/B and
// test knob, ≥ 1), default 256 MiB — at C3's 12.7 KB per instance 21,000 instances per slice,
// enough to fill the device many times over, and a bound that does not grow with the batch.
int64_t expand_cap() {
  const char* e = std::getenv("MCPX_EXPAND_MB");
  const long long v = e ? std::atoll(e) : 256;
  return (int64_t)(v < 1 ? 1 : v) << 20;
}

// A shared-matrix batch (mcpx_solve_batch_shared*) on device buffers: instance i's θ′ is
// `shared` (one copy) followed by var + i·d->theta_ld.
//   * QP family, SCHUR, one wave: the SHARED kernels read the two blocks in place;
//   * everything else: slices of at most expand_cap() bytes of materialised θ′ (theta_expand.hip)
//     in one block of the device cache, each solved by the kernels of the full-θ call before the
//     next slice overwrites it (stream order).
// Both give the bits of launch_chunks on the materialised θ′.
// `gmap` (mcpx_solve_batch_grouped*): a grouped batch — instance i's block is shared + gmap[i]·shared_ld;
// the map moves with the other per-instance pointers, and a slice may straddle group boundaries.
int launch_shared_chunks(const mcpx_desc* d, const double* shared, const double* var, const double* x0,
                         const double* y0, const double* s0, const mcpx_out* o, mcpx::KernelArgs a,
                         const SolvePlan& plan, hipStream_t st, const int32_t* gmap = nullptr,
                         int64_t shared_ld = 0) {
  const int n = d->n, m = d->m;
  if (a.family == MCPX_FAMILY_QP && a.solver == MCPX_LINSOLVE_SCHUR && !plan.wg) {
    for (int64_t b0 = 0; b0 < d->batch; b0 += wg::kChunk) {
      const int64_t nb = std::min(wg::kChunk, d->batch - b0);
      set_chunk(a, d, var, x0, y0, s0, o, b0);
      a.theta_var = a.theta;
      a.var_ld = d->theta_ld;
      a.theta = shared;
      a.theta_ld = 0;
      a.group_map = gmap ? gmap + b0 : nullptr;
      a.shared_ld = shared_ld;
      hipError_t e = specialized_enabled() ? mcpx::launch_ipm_shared_spec(n, m, a, nb, st) : hipErrorNotFound;
      if (e == hipErrorNotFound) e = mcpx::launch_ipm_shared_schur(plan.nmax, a, nb, st);
      HIP_TRY(e);
    }
    return MCPX_OK;
  }
  const int64_t ds = mcpx_theta_shared_dim(d->family, n, m), dv = mcpx_theta_var_dim(d->family, n, m);
  const int64_t ld = (ds + dv + 1) & ~(int64_t)1;  // even: every row starts 16-byte aligned
  const int64_t fit = expand_cap() / (ld * (int64_t)sizeof(double));  // instances the block holds
  const int64_t slice = std::max<int64_t>(1, std::min<int64_t>(d->batch, fit));
  double* blk = nullptr;
  HIP_TRY(dev_alloc((void**)&blk, sizeof(double) * (size_t)(slice * ld), st));
  int rc = MCPX_OK;
  mcpx_desc dd = *d;
  dd.theta_ld = ld;
  a.theta_ld = ld;
  for (int64_t b0 = 0; b0 < d->batch && rc == MCPX_OK; b0 += slice) {
    dd.batch = std::min(slice, d->batch - b0);
    const hipError_t e =
        gmap ? mcpx::launch_theta_expand_grouped(shared, shared_ld, gmap + b0, var + b0 * d->theta_ld, d->theta_ld, blk,
                                                 ld, ds, dv, dd.batch, st)
             : mcpx::launch_theta_expand(shared, var + b0 * d->theta_ld, d->theta_ld, blk, ld, ds, dv, dd.batch, st);
    if (e != hipSuccess) {
      rc = fail(MCPX_EHIP, "theta expansion launch failed: %s", hipGetErrorString(e));
      break;
    }
    const mcpx_out od = out_at(o, n, m, b0);
    rc = launch_chunks(&dd, blk, x0 ? x0 + b0 * n : nullptr, y0 ? y0 + b0 * m : nullptr, s0 ? s0 + b0 * m : nullptr,
                       &od, a, plan, st);
  }
  dev_release(blk, st);
  return rc;
}

bool outputs_ok(const mcpx_out* o) {
  return o && o->x && o->y && o->s && o->kkt_error && o->eps && o->outer_iters && o->status &&
         o->trace_len >= 0;
}

// θ buffers the host-buffer pipeline rotates through: MCPX_HOST_BUFFERS (A/B knob, 2..8,
// default 3: chunk c+1 and c+2 upload while chunk c solves).
int host_buffers() {
  const char* e = std::getenv("MCPX_HOST_BUFFERS");
  const int v = e ? std::atoi(e) : 3;
  return v < 2 ? 2 : (v > kMaxHostBufs ? kMaxHostBufs : v);
}

// Instances per pipelined chunk: MCPX_HOST_CHUNK (A/B knob, ≥ 1024, default 4096:
// profiles/r02/host_pipeline.jsonl).
int64_t host_chunk() {
  const char* e = std::getenv("MCPX_HOST_CHUNK");
  const long long v = e ? std::atoll(e) : 4096;
  return v < 1024 ? 1024 : v;
}

// One device's share of mcpx_solve_batch: instances [b0, b0+nb), pipelined in chunks
// of MCPX_HOST_CHUNK instances through NB rotating θ buffers.  θ (and warm starts) of
// every chunk go up on ONE upload stream, back to back at the full host-link rate; the
// compute stream runs chunk c once its upload is done (event), and the upload of chunk
// c + NB waits for chunk c's kernel to release its buffer (event).  Outputs land in
// whole-shard device buffers and come back once, after the last kernel.
// `shared` (mcpx_solve_batch_shared): the one matrix block of a shared-matrix batch, uploaded
// once ahead of the first chunk; `theta` is then the per-instance block (stride d->theta_ld)
// and the only part of θ′ that goes through the rotating buffers.
// `groups` (mcpx_solve_batch_grouped): `shared` is then its G blocks, packed (stride shared_dim), all
// uploaded once, and each chunk's slice of the instance → group map goes up with its θ.
int solve_shard(int dev, const mcpx_desc* d, const double* shared, const double* theta, const double* x0,
                const double* y0, const double* s0, const mcpx::KernelArgs& a, const SolvePlan& plan, mcpx_out* o,
                int64_t b0, int64_t nb, const GroupTable* groups = nullptr) {
  HIP_TRY(hipSetDevice(dev));
  int rc = check_device(dev);
  if (rc) return rc;
  const int n = d->n, m = d->m;
  const int64_t W = mask_words(m);
  PipeLease lease;
  if (const hipError_t e = lease.acquire(dev); e != hipSuccess)
    return fail(MCPX_EHIP, "stream setup: %s", hipGetErrorString(e));
  Pipe* P = lease.p;
  const int NB = host_buffers();
  const int64_t ch = std::min(host_chunk(), nb);
  const int64_t ld = d->theta_ld;
  hipStream_t cs = P->comp, us = P->up;
  AsyncBuf<double> th[kMaxHostBufs], wx[kMaxHostBufs], wy[kMaxHostBufs], ws[kMaxHostBufs];
  AsyncBuf<double> sh, x, y, s, kkt, eps;
  AsyncBuf<int32_t> outer, status, newton, gm[kMaxHostBufs];
  AsyncBuf<uint64_t> am;
  AsyncBuf<uint8_t> tr, fr;
  // declared after the buffers, so it runs before their (stream-ordered) frees on every
  // exit: no upload or kernel may still target a buffer when it returns to the cache
  struct Drain {
    hipStream_t a, b;
    ~Drain() {
      (void)hipStreamSynchronize(a);
      (void)hipStreamSynchronize(b);
    }
  } drain{us, cs};
  const int nbuf = (int)std::min<int64_t>(NB, (nb + ch - 1) / std::max<int64_t>(ch, 1));
  for (int k = 0; k < nbuf; ++k) {  // every buffer lives on the compute stream (allocated, used, freed there)
    HIP_TRY(th[k].alloc((size_t)ch * ld, cs));
    if (x0) HIP_TRY(wx[k].alloc((size_t)ch * n, cs));
    if (y0) HIP_TRY(wy[k].alloc((size_t)ch * m, cs));
    if (s0) HIP_TRY(ws[k].alloc((size_t)ch * m, cs));
    if (groups) HIP_TRY(gm[k].alloc((size_t)ch, cs));
  }
  const int64_t ds = shared ? mcpx_theta_shared_dim(d->family, n, m) : 0;
  const int64_t nsh = groups ? groups->G * ds : ds;  // doubles of the matrix block(s)
  // the last instance of a chunk: its own doubles, not the stride (strided_span) — the
  // per-instance block of a shared-matrix batch, else the whole θ of the family or the module
  const int64_t own = shared     ? mcpx_theta_var_dim(d->family, n, m)
                      : plan.mod ? (int64_t)plan.mod->meta[kMetaP]
                                 : mcpx_theta_dim(d->family, n, m);
  if (shared) HIP_TRY(sh.alloc((size_t)std::max<int64_t>(nsh, 1), cs));
  HIP_TRY(x.alloc((size_t)nb * n, cs)); HIP_TRY(y.alloc((size_t)nb * m, cs)); HIP_TRY(s.alloc((size_t)nb * m, cs));
  HIP_TRY(kkt.alloc(nb, cs)); HIP_TRY(eps.alloc(nb, cs)); HIP_TRY(outer.alloc(nb, cs));
  HIP_TRY(status.alloc(nb, cs));
  if (o->newton_iters) HIP_TRY(newton.alloc(nb, cs));
  if (o->active_mask) HIP_TRY(am.alloc((size_t)nb * W, cs));
  if (o->fail_reason) HIP_TRY(fr.alloc(nb, cs));
  const bool want_tr = o->alpha_trace && o->trace_len > 0;
  if (want_tr) {
    HIP_TRY(tr.alloc((size_t)nb * o->trace_len * 2, cs));
    HIP_TRY(hipMemsetAsync(tr.p, 254, (size_t)nb * o->trace_len * 2, cs));
  }
  // the allocations (compute stream) before the first upload into them
  HIP_TRY(hipEventRecord(P->consumed[0], cs));
  HIP_TRY(hipStreamWaitEvent(us, P->consumed[0], 0));
  // the shared block: once, on the upload stream ahead of chunk 0 (whose event covers it)
  if (shared && nsh > 0) HIP_TRY(hipMemcpyAsync(sh.p, shared, sizeof(double) * (size_t)nsh, hipMemcpyHostToDevice, us));
  for (int64_t c0 = 0, ci = 0; c0 < nb; c0 += ch, ++ci) {
    const int k = (int)(ci % nbuf);
    const int64_t cn = std::min(ch, nb - c0), g0 = b0 + c0;
    if (ci >= nbuf) HIP_TRY(hipStreamWaitEvent(us, P->consumed[k], 0));  // chunk ci - nbuf released buffer k
    HIP_TRY(hipMemcpyAsync(th[k].p, theta + g0 * ld, sizeof(double) * strided_span(cn, ld, own),
                           hipMemcpyHostToDevice, us));
    if (x0) HIP_TRY(hipMemcpyAsync(wx[k].p, x0 + g0 * n, sizeof(double) * cn * n, hipMemcpyHostToDevice, us));
    if (y0) HIP_TRY(hipMemcpyAsync(wy[k].p, y0 + g0 * m, sizeof(double) * cn * m, hipMemcpyHostToDevice, us));
    if (s0) HIP_TRY(hipMemcpyAsync(ws[k].p, s0 + g0 * m, sizeof(double) * cn * m, hipMemcpyHostToDevice, us));
    if (groups)
      HIP_TRY(hipMemcpyAsync(gm[k].p, groups->map.data() + g0, sizeof(int32_t) * cn, hipMemcpyHostToDevice, us));
    HIP_TRY(hipEventRecord(P->copied[k], us));
    HIP_TRY(hipStreamWaitEvent(cs, P->copied[k], 0));
    mcpx_out od{};
    od.x = x.p + c0 * n; od.y = y.p + c0 * m; od.s = s.p + c0 * m; od.kkt_error = kkt.p + c0; od.eps = eps.p + c0;
    od.outer_iters = outer.p + c0; od.status = status.p + c0; od.newton_iters = newton.p ? newton.p + c0 : nullptr;
    od.active_mask = am.p ? am.p + c0 * W : nullptr;
    od.alpha_trace = want_tr ? tr.p + c0 * (int64_t)o->trace_len * 2 : nullptr;
    od.trace_len = want_tr ? o->trace_len : 0;
    od.fail_reason = fr.p ? fr.p + c0 : nullptr;
    mcpx_desc dd = *d;
    dd.batch = cn;
    rc = shared ? launch_shared_chunks(&dd, sh.p, th[k].p, wx[k].p, wy[k].p, ws[k].p, &od, a, plan, cs, gm[k].p, ds)
                : launch_chunks(&dd, th[k].p, wx[k].p, wy[k].p, ws[k].p, &od, a, plan, cs);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(P->consumed[k], cs));
  }
  HIP_TRY(hipStreamSynchronize(us));
  HIP_TRY(hipStreamSynchronize(cs));
  auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
  };
  HIP_TRY(back(o->x + b0 * n, x.p, sizeof(double) * nb * n));
  HIP_TRY(back(o->y + b0 * m, y.p, sizeof(double) * nb * m));
  HIP_TRY(back(o->s + b0 * m, s.p, sizeof(double) * nb * m));
  HIP_TRY(back(o->kkt_error + b0, kkt.p, sizeof(double) * nb));
  HIP_TRY(back(o->eps + b0, eps.p, sizeof(double) * nb));
  HIP_TRY(back(o->outer_iters + b0, outer.p, sizeof(int32_t) * nb));
  HIP_TRY(back(o->status + b0, status.p, sizeof(int32_t) * nb));
  if (o->newton_iters) HIP_TRY(back(o->newton_iters + b0, newton.p, sizeof(int32_t) * nb));
  if (o->active_mask) HIP_TRY(back(o->active_mask + b0 * W, am.p, sizeof(uint64_t) * nb * W));
  if (want_tr) HIP_TRY(back(o->alpha_trace + b0 * o->trace_len * 2, tr.p, (size_t)nb * o->trace_len * 2));
  if (o->fail_reason) HIP_TRY(back(o->fail_reason + b0, fr.p, (size_t)nb));
  return MCPX_OK;
}


// Shards of a host-buffer call: one per device, or MCPX_HOST_SHARDS = k contiguous shards
// over the caller's (clamped) devices round-robin — shard g runs on device g mod
// num_devices, never on a device the caller did not ask for (a test knob that runs the
// multi-device path on a box with fewer devices).
int host_shards(int num_devices, int64_t batch) {
  const char* e = std::getenv("MCPX_HOST_SHARDS");
  const int k = e ? std::atoi(e) : 0;
  if (k <= 0) return num_devices;
  return (int)std::max<int64_t>(1, std::min<int64_t>(k, batch));
}

// Runs fn(device, b0, nb) over the contiguous shards of a host-buffer call: shard g (device
// g mod devices) gets ⌊B/G⌋ instances (+1 for g < B mod G).  One host thread per shard; a
// single shard runs on the caller's thread.  `unit` > 1 (mcpx_vjp_batch_shared_reduce): the
// shards are cut at multiples of `unit` instances, the units dealt out as the instances are.
template <class Fn>
int run_shards(int num_devices, int64_t batch, Fn&& fn, int64_t unit = 1) {
  const int avail = mcpx_device_count();
  if (avail < 1) return fail(MCPX_ENODEV, "no HIP device visible");
  const int64_t units = (batch + unit - 1) / unit;
  if (num_devices <= 0 || num_devices > avail) num_devices = avail;
  if ((int64_t)num_devices > units) num_devices = (int)units;
  const int devs = num_devices, shards = host_shards(devs, units);
  if (shards == 1) return fn(0, (int64_t)0, batch);
  std::vector<int64_t> start(shards + 1, 0);
  for (int g = 0; g < shards; ++g)
    start[g + 1] = std::min(batch, (start[g] + unit - 1) / unit * unit + unit * (units / shards + (g < units % shards ? 1 : 0)));
  std::vector<int> rcs(shards, 0);
  std::vector<std::string> errs(shards);
  std::vector<std::thread> th;
  for (int g = 0; g < shards; ++g)
    th.emplace_back([&, g] {
      rcs[g] = fn(g % devs, start[g], start[g + 1] - start[g]);
      if (rcs[g]) errs[g] = g_err;
    });
  for (auto& t : th) t.join();
  for (int g = 0; g < shards; ++g)
    if (rcs[g]) return fail(rcs[g], "device %d: %s", g, errs[g].c_str());
  return MCPX_OK;
}

// ---- sensitivities (src/AutoDiff.jl) ----------------------------------------

// mcpx_vjp_batch*, mcpx_jvp_batch*, or mcpx_cond_batch*: the JVP workgroup kernels in their
// condition-estimate mode (every size and family runs the workgroup layout: the estimate's
// solves reuse the factors in the slot).
enum SensKind { kVjp, kJvp, kCond };

// How a sensitivity call runs: one wave per instance (QP / affine, n + 2m ≤ 64: the
// register kernels of sens_kernel_impl.hpp, `nmax` wide) or one workgroup per instance
// (larger QP / affine systems in the dimension bucket `nv`, and every generated module).
// `split`: a shared-matrix batch (mcpx_vjp_batch_shared*, mcpx_jvp_batch_shared*) — the SPLIT
// kernels, which read one matrix block and write / read the per-instance block's n + m doubles.
// `dot` (with split, a JVP: mcpx_jvp_batch_shared_dot*): the kThetaSplitDot kernels, which take the
// matrix block's tangents from SensArgs::shared_dot.
struct SensPlan {
  int nmax = 0;
  bool wg = false;
  int nv = 0;
  mcpx_module* mod = nullptr;
  bool split = false;
  bool dot = false;
};

// Validates a sensitivity call; fills the scalar part of the args (the caller's pointers,
// n_partials and cotangent factors stay) and the plan.  `split`: a shared-matrix call — desc->theta_ld
// is checked as in the shared solve, a->p is the per-instance dimension n + m (the stride of the
// outputs and tangents), and the kernels read a->theta for every instance.
int prepare_sens(const mcpx_desc* d, mcpx::SensArgs* a, SensPlan* plan, SensKind kind, mcpx_module* mod,
                 bool split = false, bool dot = false) {
  if (!d) return fail(MCPX_EINVAL, "desc must be non-NULL");
  int64_t pd;
  if (const int rc = check_desc(d, mod, &pd, kSensWords, split)) return rc;
  const bool jvp = kind != kVjp;
  const int N = d->n + 2 * d->m;
  *plan = SensPlan{};
  plan->mod = mod;
  plan->split = split;
  plan->dot = split && dot && kind == kJvp;
  if (mod) {
    if (!mod->has(jvp ? MCPX_MODULE_JVP : MCPX_MODULE_VJP))
      return fail(MCPX_EUNSUPPORTED, "the generated module has no %s kernel (n=%d m=%d: not even a 4-column LU panel of "
                  "its %d-row system fits the LDS)", jvp ? "JVP" : "VJP", d->n, d->m, jvp ? N : d->n + d->m);
    plan->wg = true;
  } else if (N <= MCPX_MAX_WG_KKT_DIM) {
    if (N <= MCPX_MAX_KKT_DIM && kind != kCond) {
      plan->nmax = pick_nmax(N);
    } else {
      plan->wg = true;
      plan->nv = pick_wg_bucket(N);
    }
  } else {
    return fail(MCPX_EUNSUPPORTED, "sensitivities need n + 2m <= %d (got n=%d m=%d)", MCPX_MAX_WG_KKT_DIM, d->n, d->m);
  }
  a->theta_ld = split ? 0 : d->theta_ld;
  a->p = pd;
  a->n = d->n;
  a->m = d->m;
  a->family = d->family;
  a->mode = kind == kCond ? 1 : 0;
  return MCPX_OK;
}

// The argument checks after prepare_sens; an empty batch reads nothing and passes.
// `dot` (mcpx_jvp_batch_shared_dot*): shared_dot is the required tangent, theta_dot (var_dot) may be NULL.
int sens_inputs_ok(const mcpx_desc* d, const mcpx::SensArgs& a, bool dot = false) {
  if (a.n_partials < 0) return fail(MCPX_EINVAL, "negative n_partials");
  if (d->batch == 0) return MCPX_OK;
  if (!a.theta || !a.out) return fail(MCPX_EINVAL, "theta and the output array must be non-NULL");
  if ((d->n > 0 && !a.x) || (d->m > 0 && (!a.y || !a.s)))
    return fail(MCPX_EINVAL, "solution arrays x/y/s must be non-NULL");
  if (a.n_partials > 0 && dot && !a.shared_dot) return fail(MCPX_EINVAL, "shared_dot is NULL");
  if (a.n_partials > 0 && !dot && !a.theta_dot) return fail(MCPX_EINVAL, "theta_dot is NULL");
  return MCPX_OK;
}

// Doubles of one instance's output: rcond, zdot [K × (n+2m)] or dtheta [p].
int64_t sens_out_len(const mcpx::SensArgs& a, bool jvp) {
  return a.mode == 1 ? 1 : (jvp ? (int64_t)a.n_partials * (a.n + 2 * a.m) : a.p);
}

// The args of the chunk that starts at instance b0 (the counterpart of set_chunk).
mcpx::SensArgs sens_chunk(mcpx::SensArgs a, bool jvp, int64_t b0) {
  const int n = a.n, m = a.m;
  a.out += b0 * sens_out_len(a, jvp);
  a.theta += b0 * a.theta_ld;
  a.x += b0 * n;
  a.y += b0 * m;
  a.s += b0 * m;
  if (a.gx) a.gx += b0 * n;
  if (a.gy) a.gy += b0 * m;
  if (a.gs) a.gs += b0 * m;
  if (a.theta_dot) a.theta_dot += b0 * a.n_partials * a.p;
  if (a.status) a.status += b0;
  if (a.group_map) a.group_map += b0;
  return a;
}

// Workgroup-per-instance sensitivity launch (sens_wg_impl.hpp): the slot holds [K | rhs]
// (and a module's Jacobian blocks and ∇F_θ, wg_layout.h).
int launch_sens_wg_impl(bool jvp, const mcpx_desc* d, const mcpx::SensArgs& a, const SensPlan& plan, hipStream_t st) {
  GridKernel k;
  if (plan.mod) {
    const char* name = jvp ? "mcpx_nl_jvp_wg" : "mcpx_nl_vjp_wg";
    int dev = 0;
    const int rc = module_function(plan.mod, name, name, &k.f, &dev);
    if (rc) return rc;
  } else {
    k.sym = plan.dot     ? mcpx::sens_wg_shared_dot_kernel(a.family, plan.nv)
            : plan.split ? mcpx::sens_wg_shared_kernel(a.family, jvp, plan.nv)
                         : mcpx::sens_wg_kernel(a.family, jvp, plan.nv);
    if (!k.sym) return fail(MCPX_EUNSUPPORTED, "no workgroup sensitivity kernel for family %d, dim %d", a.family, plan.nv);
  }
  wg::WgSensArgs w = wg::sens_layout(jvp, a.mode, a.n, a.m, a.p, a.n_partials,
                                     plan.mod ? plan.mod->meta[kMetaBlock] : wg::kNoModule);
  return launch_persistent(k, -1, d->batch, w, wg::kSensWorkCap, st, "workgroup sensitivity", [&](int64_t b0, int grid) {
    w.s = sens_chunk(a, jvp, b0);
    if (plan.mod) return launch_module(k.f, grid, k.threads, &w, st);
    if (plan.dot) return mcpx::launch_sens_wg_shared_dot(a.family, plan.nv, w, grid, st);
    return plan.split ? mcpx::launch_sens_wg_shared(a.family, jvp, plan.nv, w, grid, st)
                      : mcpx::launch_sens_wg(a.family, jvp, plan.nv, w, grid, st);
  });
}

// Enqueue VJP (jvp = false) or JVP launches over the batch: the one-wave kernels in
// chunks of 2^30 instances, or the workgroup kernels.
int launch_sens(bool jvp, const mcpx_desc* d, const mcpx::SensArgs& a, const SensPlan& plan, hipStream_t st) {
  if (plan.wg) return launch_sens_wg_impl(jvp, d, a, plan, st);
  for (int64_t b0 = 0; b0 < d->batch; b0 += wg::kChunk) {
    const int64_t nb = std::min(wg::kChunk, d->batch - b0);
    const mcpx::SensArgs c = sens_chunk(a, jvp, b0);
    // the VJP factors the slack-eliminated (n+m)-dim system, the JVP the full n+2m
    if (plan.dot)
      HIP_TRY(mcpx::launch_jvp_shared_dot(plan.nmax, c, nb, st));
    else if (plan.split)
      HIP_TRY(jvp ? mcpx::launch_jvp_shared(plan.nmax, c, nb, st)
                  : mcpx::launch_vjp_shared(pick_nmax(a.n + a.m), c, nb, st));
    else
      HIP_TRY(jvp ? mcpx::launch_jvp(plan.nmax, c, nb, st) : mcpx::launch_vjp(pick_nmax(a.n + a.m), c, nb, st));
  }
  return MCPX_OK;
}

// One device's share [b0, b0+nb) of a host-buffer sensitivity call (`a`: host pointers).
// A shared-matrix call (plan.split) uploads its one matrix block, no per-instance θ, and brings
// back a.p = n + m doubles per instance (the VJP; rcond: one double).  plan.dot: the one
// [K × shared_dim] block of matrix tangents goes up once as well.
// `groups` (mcpx_vjp_batch_grouped): a.theta is the G packed blocks, all uploaded, with the shard's
// slice of the instance → group map.
int sens_shard(bool jvp, int dev, const mcpx_desc* d, const mcpx::SensArgs& a, const SensPlan& plan, int64_t b0,
               int64_t nb, const GroupTable* groups = nullptr) {
  HIP_TRY(hipSetDevice(dev));
  int rc = check_device(dev);
  if (rc) return rc;
  const int n = d->n, m = d->m;
  DevBuf<double> th, dx, dy, ds, dgx, dgy, dgs, dtd, dsd, dout;
  DevBuf<int32_t> dst, dmap;
  auto up = [&](DevBuf<double>& b, const double* h, size_t per) -> hipError_t {
    if (!h || !per || !nb) return hipSuccess;
    hipError_t e = b.alloc((size_t)nb * per);
    return e != hipSuccess ? e : hipMemcpy(b.p, h + b0 * per, sizeof(double) * nb * per, hipMemcpyHostToDevice);
  };
  if (plan.split) {
    const int64_t ds = mcpx_theta_shared_dim(d->family, n, m);
    const int64_t nsh = groups ? groups->G * ds : ds;
    HIP_TRY(th.alloc((size_t)std::max<int64_t>(nsh, 1)));
    if (nsh > 0) HIP_TRY(hipMemcpy(th.p, a.theta, sizeof(double) * (size_t)nsh, hipMemcpyHostToDevice));
    if (groups && nb) {
      HIP_TRY(dmap.alloc((size_t)nb));
      HIP_TRY(hipMemcpy(dmap.p, groups->map.data() + b0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice));
    }
    const size_t nsd = plan.dot ? (size_t)a.n_partials * (size_t)ds : 0;
    if (nsd) {
      HIP_TRY(dsd.alloc(nsd));
      HIP_TRY(hipMemcpy(dsd.p, a.shared_dot, sizeof(double) * nsd, hipMemcpyHostToDevice));
    }
  } else if (nb) {  // θ at the caller's stride; the last instance's a.p doubles end the copy
    HIP_TRY(th.alloc((size_t)nb * (size_t)d->theta_ld));
    HIP_TRY(hipMemcpy(th.p, a.theta + b0 * d->theta_ld, sizeof(double) * strided_span(nb, d->theta_ld, a.p),
                      hipMemcpyHostToDevice));
  }
  HIP_TRY(up(dx, a.x, n)); HIP_TRY(up(dy, a.y, m)); HIP_TRY(up(ds, a.s, m));
  HIP_TRY(up(dgx, a.gx, n)); HIP_TRY(up(dgy, a.gy, m)); HIP_TRY(up(dgs, a.gs, m));
  HIP_TRY(up(dtd, a.theta_dot, (size_t)a.n_partials * a.p));
  const size_t per_out = (size_t)sens_out_len(a, jvp);
  HIP_TRY(dout.alloc((size_t)nb * per_out));
  if (a.status) HIP_TRY(dst.alloc(nb));
  mcpx_desc dd = *d;
  dd.batch = nb;
  mcpx::SensArgs da = a;  // the same call on the shard's device buffers
  da.theta = th.p;
  // empty x/y blocks (n = 0 or m = 0) still need a valid base pointer
  da.x = dx.p ? dx.p : th.p;
  da.y = dy.p ? dy.p : th.p;
  da.s = ds.p ? ds.p : th.p;
  da.gx = dgx.p;
  da.gy = dgy.p;
  da.gs = dgs.p;
  da.theta_dot = dtd.p;
  da.shared_dot = dsd.p ? dsd.p : th.p;  // (an empty matrix block, n = 0: never read)
  // an empty output (p = 0, or K = 0) still needs a valid base pointer
  da.out = dout.p ? dout.p : (double*)th.p;
  da.status = dst.p;
  da.group_map = dmap.p;
  da.shared_ld = groups ? mcpx_theta_shared_dim(d->family, n, m) : 0;
  if ((rc = launch_sens(jvp, &dd, da, plan, nullptr))) {
    (void)hipDeviceSynchronize();  // nothing may still run on the buffers freed on return
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (per_out) HIP_TRY(hipMemcpy(a.out + b0 * per_out, dout.p, sizeof(double) * nb * per_out, hipMemcpyDeviceToHost));
  if (a.status) HIP_TRY(hipMemcpy(a.status + b0, dst.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  return MCPX_OK;
}

// The device-buffer sensitivity entries (`a`: the caller's pointers, n_partials): enqueued
// on `stream` of the current device.  `split`: a.theta is the matrix block of a shared-matrix batch.
int sens_device(SensKind kind, mcpx_module* mod, const mcpx_desc* d, mcpx::SensArgs a, void* stream,
                bool split = false, bool dot = false) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_sens(d, &a, &plan, kind, mod, split, dot))) return rc;
  if ((rc = sens_inputs_ok(d, a, dot)) || d->batch == 0) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  // empty x/y blocks (n = 0 or m = 0) still need a valid base pointer
  if (!a.x) a.x = a.theta;
  if (!a.y) a.y = a.theta;
  if (!a.s) a.s = a.theta;
  return launch_sens(kind != kVjp, d, a, plan, (hipStream_t)stream);
}

// The host-buffer sensitivity entries: contiguous shards over the devices.
int sens_host(SensKind kind, mcpx_module* mod, const mcpx_desc* d, mcpx::SensArgs a, int num_devices,
              bool split = false, bool dot = false) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_sens(d, &a, &plan, kind, mod, split, dot))) return rc;
  if ((rc = sens_inputs_ok(d, a, dot)) || d->batch == 0) return rc;
  return run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
    return sens_shard(kind != kVjp, dev, d, a, plan, b0, nb);
  });
}

// The pointer part of a sensitivity call's args, as the extern "C" entries receive it.
mcpx::SensArgs sens_args(const double* theta, const double* x, const double* y, const double* s, double* out,
                         int32_t* status) {
  mcpx::SensArgs a{};
  a.theta = theta;
  a.x = x;
  a.y = y;
  a.s = s;
  a.out = out;
  a.status = status;
  return a;
}

// ---- the reduced gradient of the shared block (mcpx_vjp_batch_shared_reduce*) --------------

// Bytes of chunk partials one launch of shared_reduce_partial may leave behind: past it the
// chunks go through the block in groups, each folded (or copied out) before the next
// overwrites it, so the scratch does not grow with B · shared_dim.
// MCPX_REDUCE_CAP_KB (test knob, ≥ 1): the cap in KiB, so that a small batch runs in groups.
int64_t reduce_partial_cap() {
  const char* e = std::getenv("MCPX_REDUCE_CAP_KB");
  const long long v = e ? std::atoll(e) : 32ll << 10;
  return (int64_t)(v < 1 ? 1 : v) << 10;
}

// The checks of the reduce entries after prepare_sens (dvar and status may be NULL).
int reduce_inputs_ok(const mcpx_desc* d, const mcpx::SensArgs& a, const double* dshared, const int64_t* used) {
  if (!dshared || !used) return fail(MCPX_EINVAL, "dshared and used must be non-NULL");
  if (d->batch == 0) return MCPX_OK;
  if (!a.theta) return fail(MCPX_EINVAL, "theta_shared must be non-NULL");
  if ((d->n > 0 && !a.x) || (d->m > 0 && (!a.y || !a.s)))
    return fail(MCPX_EINVAL, "solution arrays x/y/s must be non-NULL");
  return MCPX_OK;
}

// The split pullback of `a` (device pointers; a.out / a.status NULL: into a pool block), then
// the chunk partials of Σ_b ∂shared, all on `st`.  d->batch instances that start a chunk.
// hpart == NULL: folded on the device into dshared / used (device pointers).  Otherwise the
// partials and counts of every chunk are copied to hpart [chunks × ds] / hcount [chunks] (host),
// for the caller to fold across shards.
int launch_shared_reduce(const mcpx_desc* d, mcpx::SensArgs a, const SensPlan& plan, const uint8_t* skip,
                         double* dshared, int64_t* used, double* hpart, int64_t* hcount, hipStream_t st) {
  const int n = d->n, m = d->m;
  const int64_t B = d->batch, ds = mcpx_theta_shared_dim(d->family, n, m);
  const int64_t nch = (B + MCPX_REDUCE_CHUNK - 1) / MCPX_REDUCE_CHUNK;
  const int64_t group = std::max<int64_t>(1, std::min(nch, reduce_partial_cap() / (std::max<int64_t>(ds, 1) * 8)));
  AsyncBuf<double> own_dvar, part;
  AsyncBuf<int32_t> own_status;
  AsyncBuf<int64_t> count;
  if (!a.out) {
    HIP_TRY(own_dvar.alloc((size_t)B * (n + m), st));
    a.out = own_dvar.p;
  }
  if (!a.status) {
    HIP_TRY(own_status.alloc((size_t)B, st));
    a.status = own_status.p;
  }
  HIP_TRY(part.alloc((size_t)(group * std::max<int64_t>(ds, 1)), st));
  HIP_TRY(count.alloc((size_t)group, st));
  if (const int rc = launch_sens(false, d, a, plan, st)) return rc;
  mcpx::ReduceArgs r{};
  r.x = a.x;
  r.y = a.y;
  r.dvar = a.out;
  r.status = a.status;
  r.skip = skip;
  r.part = part.p;
  r.count = count.p;
  r.batch = B;
  r.ds = ds;
  r.n = n;
  r.m = m;
  r.family = d->family;
  for (int64_t c0 = 0; c0 < nch; c0 += group) {
    const int64_t nc = std::min(group, nch - c0);
    r.chunk0 = c0;
    HIP_TRY(mcpx::launch_shared_reduce_partial(r, nc, st));
    if (!hpart) {
      HIP_TRY(mcpx::launch_shared_reduce_fold(part.p, count.p, nc, ds, c0 == 0, dshared, used, st));
    } else {  // stream-ordered: both copies are done before the next group's kernel starts
      if (ds > 0)
        HIP_TRY(hipMemcpyAsync(hpart + c0 * ds, part.p, sizeof(double) * (size_t)(nc * ds), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(hcount + c0, count.p, sizeof(int64_t) * (size_t)nc, hipMemcpyDeviceToHost, st));
    }
  }
  return MCPX_OK;
}

// What the reduce entries take beyond a split pullback's SensArgs.
struct ReduceCall {
  const uint8_t* skip;
  double* dshared;
  int64_t* used;
};

int shared_reduce_device(const mcpx_desc* d, mcpx::SensArgs a, const ReduceCall& c, void* stream) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_sens(d, &a, &plan, kVjp, nullptr, true))) return rc;
  if ((rc = reduce_inputs_ok(d, a, c.dshared, c.used))) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (d->batch == 0) {  // the empty sum: all bits zero is +0.0 and 0
    const int64_t ds = mcpx_theta_shared_dim(d->family, d->n, d->m);
    if (ds > 0) HIP_TRY(hipMemsetAsync(c.dshared, 0, sizeof(double) * (size_t)ds, st));
    HIP_TRY(hipMemsetAsync(c.used, 0, sizeof(int64_t), st));
    return MCPX_OK;
  }
  // empty x/y blocks (n = 0 or m = 0) still need a valid base pointer
  if (!a.x) a.x = a.theta;
  if (!a.y) a.y = a.theta;
  if (!a.s) a.s = a.theta;
  return launch_shared_reduce(d, a, plan, c.skip, c.dshared, c.used, nullptr, nullptr, st);
}

// One device's share [b0, b0 + nb) of the host call, b0 a multiple of MCPX_REDUCE_CHUNK: the
// chunk partials and counts of the shard into hpart / hcount at its global chunk index.
int shared_reduce_shard(int dev, const mcpx_desc* d, const mcpx::SensArgs& a, const SensPlan& plan,
                        const ReduceCall& c, double* hpart, int64_t* hcount, int64_t b0, int64_t nb) {
  HIP_TRY(hipSetDevice(dev));
  int rc = check_device(dev);
  if (rc) return rc;
  const int n = d->n, m = d->m;
  const int64_t ds = mcpx_theta_shared_dim(d->family, n, m);
  DevBuf<double> th, dx, dy, dsl, dgx, dgy, dgs, dout;
  DevBuf<int32_t> dst;
  DevBuf<uint8_t> dskip;
  auto up = [&](DevBuf<double>& b, const double* h, size_t per) -> hipError_t {
    if (!h || !per) return hipSuccess;
    hipError_t e = b.alloc((size_t)nb * per);
    return e != hipSuccess ? e : hipMemcpy(b.p, h + b0 * per, sizeof(double) * nb * per, hipMemcpyHostToDevice);
  };
  HIP_TRY(th.alloc((size_t)std::max<int64_t>(ds, 1)));
  if (ds > 0) HIP_TRY(hipMemcpy(th.p, a.theta, sizeof(double) * (size_t)ds, hipMemcpyHostToDevice));
  HIP_TRY(up(dx, a.x, n)); HIP_TRY(up(dy, a.y, m)); HIP_TRY(up(dsl, a.s, m));
  HIP_TRY(up(dgx, a.gx, n)); HIP_TRY(up(dgy, a.gy, m)); HIP_TRY(up(dgs, a.gs, m));
  if (c.skip) {
    HIP_TRY(dskip.alloc((size_t)nb));
    HIP_TRY(hipMemcpy(dskip.p, c.skip + b0, (size_t)nb, hipMemcpyHostToDevice));
  }
  if (a.out) HIP_TRY(dout.alloc((size_t)nb * (n + m)));
  if (a.status) HIP_TRY(dst.alloc((size_t)nb));
  mcpx_desc dd = *d;
  dd.batch = nb;
  mcpx::SensArgs da = a;  // the same call on the shard's device buffers
  da.theta = th.p;
  da.x = dx.p ? dx.p : th.p;
  da.y = dy.p ? dy.p : th.p;
  da.s = dsl.p ? dsl.p : th.p;
  da.gx = dgx.p;
  da.gy = dgy.p;
  da.gs = dgs.p;
  da.out = dout.p;
  da.status = dst.p;
  const int64_t c0 = b0 / MCPX_REDUCE_CHUNK;
  rc = launch_shared_reduce(&dd, da, plan, dskip.p, nullptr, nullptr, hpart + c0 * ds, hcount + c0, nullptr);
  if (rc) {
    (void)hipDeviceSynchronize();  // nothing may still run on the buffers freed on return
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (a.out) HIP_TRY(hipMemcpy(a.out + b0 * (n + m), dout.p, sizeof(double) * nb * (n + m), hipMemcpyDeviceToHost));
  if (a.status) HIP_TRY(hipMemcpy(a.status + b0, dst.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  return MCPX_OK;
}

int shared_reduce_host(const mcpx_desc* d, mcpx::SensArgs a, const ReduceCall& c, int num_devices) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_sens(d, &a, &plan, kVjp, nullptr, true))) return rc;
  if ((rc = reduce_inputs_ok(d, a, c.dshared, c.used))) return rc;
  const int64_t ds = mcpx_theta_shared_dim(d->family, d->n, d->m);
  const int64_t nch = (d->batch + MCPX_REDUCE_CHUNK - 1) / MCPX_REDUCE_CHUNK;
  std::vector<double> hpart;
  std::vector<int64_t> hcount((size_t)nch, 0);
  if (nch > 0) {
    if (mcpx_device_count() < 1) return fail(MCPX_ENODEV, "no HIP device visible");
    hpart.resize((size_t)(nch * ds));
    rc = run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
      return shared_reduce_shard(dev, d, a, plan, c, hpart.data(), hcount.data(), b0, nb);
    }, MCPX_REDUCE_CHUNK);
    if (rc) return rc;
  }
  // the fold of shared_reduce_fold, over every shard's chunks in global order
  int64_t u = 0;
  for (int64_t e = 0; e < ds; ++e) c.dshared[e] = 0.0;
  for (int64_t k = 0; k < nch; ++k) {
    const double* p = hpart.data() + k * ds;
    for (int64_t e = 0; e < ds; ++e) c.dshared[e] = c.dshared[e] + p[e];
    u += hcount[(size_t)k];
  }
  *c.used = u;
  return MCPX_OK;
}

// mcpx_solve_batch_device / mcpx_solve_batch_module_device (mod = nullptr: QP / affine kernels).
int solve_device_impl(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x0,
                      const double* y0, const double* s0, const mcpx_params* prm, const mcpx_out* o,
                      void* stream) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  int rc = prepare(d, prm, &a, &plan, mod);
  if (rc) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  if (d->batch == 0) return MCPX_OK;
  if (!theta) return fail(MCPX_EINVAL, "theta is NULL");
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  return launch_chunks(d, theta, x0, y0, s0, o, a, plan, (hipStream_t)stream);
}

// mcpx_solve_vjp_batch_device: the solve kernels with the pullback in their epilogue
// (ipm_inst_fused.hip) where they exist, else the solve then the VJP launches.
int solve_vjp_device_impl(const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
                          const double* s0, const mcpx_params* prm, const mcpx_out* o, const mcpx_cotangent* ct,
                          double* dtheta, int32_t* vstat, void* stream) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  int rc = prepare(d, prm, &a, &plan, nullptr);
  if (rc) return rc;
  mcpx::SensArgs sa{};
  SensPlan splan;
  if ((rc = prepare_sens(d, &sa, &splan, kVjp, nullptr))) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  if (!ct) return fail(MCPX_EINVAL, "the cotangent must be non-NULL");
  if (d->batch == 0) return MCPX_OK;
  if (!theta || !dtheta) return fail(MCPX_EINVAL, "theta and dtheta must be non-NULL");
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int n = d->n, m = d->m;
  if (!plan.wg && specialized_enabled() && mcpx::has_fused_vjp(a.family, a.solver, n, m)) {
    a.ct_ax = ct->ax;
    a.ct_ay = ct->ay;
    a.ct_as = ct->as;
    for (int64_t b0 = 0; b0 < d->batch; b0 += wg::kChunk) {
      const int64_t nb = std::min(wg::kChunk, d->batch - b0);
      set_chunk(a, d, theta, x0, y0, s0, o, b0);
      a.vjp_dtheta = dtheta + b0 * sa.p;
      a.vjp_status = vstat ? vstat + b0 : nullptr;
      a.ct_bx = ct->bx ? ct->bx + b0 * n : nullptr;
      a.ct_by = ct->by ? ct->by + b0 * m : nullptr;
      a.ct_bs = ct->bs ? ct->bs + b0 * m : nullptr;
      HIP_TRY(mcpx::launch_ipm_fused_vjp(a.family, a.solver, n, m, a, nb, st));
    }
    return MCPX_OK;
  }
  if ((rc = launch_chunks(d, theta, x0, y0, s0, o, a, plan, st))) return rc;
  sa.theta = theta;
  sa.x = o->x;
  sa.y = o->y;
  sa.s = o->s;
  sa.gx = ct->bx;
  sa.gy = ct->by;
  sa.gs = ct->bs;
  sa.out = dtheta;
  sa.status = vstat;
  sa.ga_x = ct->ax;
  sa.ga_y = ct->ay;
  sa.ga_s = ct->as;
  return launch_sens(false, d, sa, splan, st);
}

// mcpx_solve_vjp_batch_shared_device: the SHARED solve kernels with the pullback in their epilogue
// (ipm_inst_shared_fused.hip) where they exist, else the shared solve (in place or through the
// expansion block, launch_shared_chunks) then the split VJP launches on its outputs — the
// pullback needs the matrix block only, never the expansion.
int solve_vjp_shared_device_impl(const mcpx_desc* d, const double* shared, const double* var, const double* x0,
                                 const double* y0, const double* s0, const mcpx_params* prm, const mcpx_out* o,
                                 const mcpx_cotangent* ct, double* dvar, int32_t* vstat, void* stream) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  int rc = prepare(d, prm, &a, &plan, nullptr, true);
  if (rc) return rc;
  mcpx::SensArgs sa{};
  SensPlan splan;
  if ((rc = prepare_sens(d, &sa, &splan, kVjp, nullptr, true))) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  if (!ct) return fail(MCPX_EINVAL, "the cotangent must be non-NULL");
  if (d->batch == 0) return MCPX_OK;
  if (!shared || !var || !dvar) return fail(MCPX_EINVAL, "theta_shared, theta_var and dvar must be non-NULL");
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int n = d->n, m = d->m;
  if (!plan.wg && specialized_enabled() && mcpx::has_fused_vjp(a.family, a.solver, n, m)) {
    a.ct_ax = ct->ax;
    a.ct_ay = ct->ay;
    a.ct_as = ct->as;
    for (int64_t b0 = 0; b0 < d->batch; b0 += wg::kChunk) {
      const int64_t nb = std::min(wg::kChunk, d->batch - b0);
      set_chunk(a, d, var, x0, y0, s0, o, b0);
      a.theta_var = a.theta;
      a.var_ld = d->theta_ld;
      a.theta = shared;
      a.theta_ld = 0;
      a.vjp_dtheta = dvar + b0 * sa.p;
      a.vjp_status = vstat ? vstat + b0 : nullptr;
      a.ct_bx = ct->bx ? ct->bx + b0 * n : nullptr;
      a.ct_by = ct->by ? ct->by + b0 * m : nullptr;
      a.ct_bs = ct->bs ? ct->bs + b0 * m : nullptr;
      HIP_TRY(mcpx::launch_ipm_shared_fused_vjp(n, m, a, nb, st));
    }
    return MCPX_OK;
  }
  if ((rc = launch_shared_chunks(d, shared, var, x0, y0, s0, o, a, plan, st))) return rc;
  sa.theta = shared;
  sa.x = o->x;
  sa.y = o->y;
  sa.s = o->s;
  sa.gx = ct->bx;
  sa.gy = ct->by;
  sa.gs = ct->bs;
  sa.out = dvar;
  sa.status = vstat;
  sa.ga_x = ct->ax;
  sa.ga_y = ct->ay;
  sa.ga_s = ct->as;
  return launch_sens(false, d, sa, splan, st);
}

// mcpx_solve_batch / mcpx_solve_batch_module: contiguous shards over the devices.
int solve_host_impl(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x0,
                    const double* y0, const double* s0, const mcpx_params* prm, int num_devices,
                    mcpx_out* o) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  int rc = prepare(d, prm, &a, &plan, mod);
  if (rc) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  if (d->batch == 0) return MCPX_OK;
  if (!theta) return fail(MCPX_EINVAL, "theta is NULL");
  return run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
    return solve_shard(dev, d, nullptr, theta, x0, y0, s0, a, plan, o, b0, nb);
  });
}

// mcpx_solve_batch_shared[_device]: the checks of the full-θ calls with the per-instance
// dimension in θ′'s place (a generated module's θ is the user's own: MCPX_EINVAL).
int prepare_shared(const mcpx_desc* d, const double* shared, const double* var, const mcpx_params* prm,
                   const mcpx_out* o, mcpx::KernelArgs* a, SolvePlan* plan, bool* empty) {
  const int rc = prepare(d, prm, a, plan, nullptr, true);
  if (rc) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  *empty = d->batch == 0;
  if (!*empty && (!shared || !var)) return fail(MCPX_EINVAL, "theta_shared or theta_var is NULL");
  return MCPX_OK;
}

// ---- the grouped entries -----------------------------------------------------------------------

// What the grouped entries take in the shared block's place.
struct GroupCall {
  const double* shared;
  int64_t shared_ld;
  int32_t G;
  const int64_t* off;
};

// mcpx_solve_batch_grouped[_device]: the checks of the shared solve, then the groups'.
int prepare_grouped(const mcpx_desc* d, const GroupCall& g, const double* var, const mcpx_params* prm,
                    const mcpx_out* o, mcpx::KernelArgs* a, SolvePlan* plan, bool* empty) {
  int rc = prepare(d, prm, a, plan, nullptr, true);
  if (rc) return rc;
  if ((rc = check_groups(d, g.shared, g.shared_ld, g.G, g.off, mcpx_theta_shared_dim(d->family, d->n, d->m)))) return rc;
  if (!outputs_ok(o)) return fail(MCPX_EINVAL, "required output arrays missing");
  *empty = d->batch == 0;
  if (!*empty && !var) return fail(MCPX_EINVAL, "theta_var is NULL");
  return MCPX_OK;
}

// The split pullback's preparation and checks for a grouped call.
int prepare_grouped_sens(const mcpx_desc* d, const GroupCall& g, mcpx::SensArgs* a, SensPlan* plan) {
  int rc = prepare_sens(d, a, plan, kVjp, nullptr, true);
  if (rc) return rc;
  return check_groups(d, g.shared, g.shared_ld, g.G, g.off, mcpx_theta_shared_dim(d->family, d->n, d->m));
}

int grouped_vjp_device(const mcpx_desc* d, const GroupCall& g, mcpx::SensArgs a, void* stream) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_grouped_sens(d, g, &a, &plan))) return rc;
  if ((rc = sens_inputs_ok(d, a)) || d->batch == 0) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  GroupTable t;
  build_groups(d, g.shared, g.shared_ld, g.G, g.off, 0, false, false, &t);
  DevGroups dg;
  HIP_TRY(dg.upload(t, st));
  a.group_map = dg.map;
  a.shared_ld = g.shared_ld;
  if (!a.x) a.x = a.theta;
  if (!a.y) a.y = a.theta;
  if (!a.s) a.s = a.theta;
  return launch_sens(false, d, a, plan, st);
}

int grouped_vjp_host(const mcpx_desc* d, const GroupCall& g, mcpx::SensArgs a, int num_devices) {
  SensPlan plan;
  int rc;
  if ((rc = prepare_grouped_sens(d, g, &a, &plan))) return rc;
  if ((rc = sens_inputs_ok(d, a)) || d->batch == 0) return rc;
  GroupTable t;
  build_groups(d, g.shared, g.shared_ld, g.G, g.off, mcpx_theta_shared_dim(d->family, d->n, d->m), true, false, &t);
  if (!t.packed.empty()) a.theta = t.packed.data();
  return run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
    return sens_shard(false, dev, d, a, plan, b0, nb, &t);
  });
}

// The grouped counterpart of launch_shared_reduce: the split pullback of `a` (device pointers whose
// element 0 is instance inst0; a.group_map / a.shared_ld set), then the partials of the chunks
// [c_lo, c_hi) of `t`, whose rows sit at dchunks[c − c_lo].  hpart == NULL: folded on the device into
// dshared / used (zeroed by the caller; dcbase: t.cbase on the device).  Otherwise every chunk's
// partial and count go to hpart [· × ds] / hcount at its chunk index of the whole batch.
int launch_grouped_reduce(const mcpx_desc* d, mcpx::SensArgs a, const SensPlan& plan, const uint8_t* skip,
                          const GroupTable& t, const mcpx::GroupChunk* dchunks, const int64_t* dcbase, int64_t c_lo,
                          int64_t c_hi, int64_t inst0, double* dshared, int64_t dshared_ld, int64_t* used, double* hpart,
                          int64_t* hcount, hipStream_t st) {
  const int n = d->n, m = d->m;
  const int64_t B = d->batch, ds = mcpx_theta_shared_dim(d->family, n, m), nch = c_hi - c_lo;
  const int64_t portion = std::max<int64_t>(1, std::min(nch, reduce_partial_cap() / (std::max<int64_t>(ds, 1) * 8)));
  AsyncBuf<double> own_dvar, part;
  AsyncBuf<int32_t> own_status;
  AsyncBuf<int64_t> count;
  if (!a.out) {
    HIP_TRY(own_dvar.alloc((size_t)B * (n + m), st));
    a.out = own_dvar.p;
  }
  if (!a.status) {
    HIP_TRY(own_status.alloc((size_t)B, st));
    a.status = own_status.p;
  }
  HIP_TRY(part.alloc((size_t)(portion * std::max<int64_t>(ds, 1)), st));
  HIP_TRY(count.alloc((size_t)portion, st));
  if (const int rc = launch_sens(false, d, a, plan, st)) return rc;
  mcpx::GroupReduceArgs r{};
  r.r.x = a.x;
  r.r.y = a.y;
  r.r.dvar = a.out;
  r.r.status = a.status;
  r.r.skip = skip;
  r.r.part = part.p;
  r.r.count = count.p;
  r.r.batch = B;
  r.r.ds = ds;
  r.r.n = n;
  r.r.m = m;
  r.r.family = d->family;
  r.chunks = dchunks;
  r.inst0 = inst0;
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += portion) {  // a portion may end inside a group: its chain goes on
    const int64_t nc = std::min(portion, c_hi - c0);
    r.r.chunk0 = c0 - c_lo;
    HIP_TRY(mcpx::launch_grouped_reduce_partial(r, nc, st));
    if (!hpart) {
      HIP_TRY(mcpx::launch_grouped_reduce_fold(part.p, count.p, c0, nc, dcbase, t.chunks[(size_t)c0].group,
                                               (int64_t)t.chunks[(size_t)(c0 + nc - 1)].group + 1, ds, dshared,
                                               dshared_ld, used, st));
    } else {  // stream-ordered: both copies are done before the next portion's kernel starts
      if (ds > 0)
        HIP_TRY(hipMemcpyAsync(hpart + c0 * ds, part.p, sizeof(double) * (size_t)(nc * ds), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(hcount + c0, count.p, sizeof(int64_t) * (size_t)nc, hipMemcpyDeviceToHost, st));
    }
  }
  return MCPX_OK;
}

// What the grouped reduce entries take beyond a grouped pullback.
struct GroupReduceCall {
  const uint8_t* skip;
  double* dshared;
  int64_t dshared_ld;
  int64_t* used;
};

int grouped_reduce_checks(const mcpx_desc* d, const GroupCall& g, const GroupReduceCall& c, mcpx::SensArgs* a,
                          SensPlan* plan) {
  int rc;
  if ((rc = prepare_grouped_sens(d, g, a, plan))) return rc;
  if (c.dshared_ld < mcpx_theta_shared_dim(d->family, d->n, d->m))
    return fail(MCPX_EINVAL, "dshared_ld %lld < shared dimension", (long long)c.dshared_ld);
  if (!c.dshared || !c.used) return fail(MCPX_EINVAL, "dshared and used must be non-NULL");
  if (d->batch > 0 && ((d->n > 0 && !a->x) || (d->m > 0 && (!a->y || !a->s))))
    return fail(MCPX_EINVAL, "solution arrays x/y/s must be non-NULL");
  return MCPX_OK;
}

int grouped_reduce_device(const mcpx_desc* d, const GroupCall& g, mcpx::SensArgs a, const GroupReduceCall& c,
                          void* stream) {
  SensPlan plan;
  int rc;
  if ((rc = grouped_reduce_checks(d, g, c, &a, &plan))) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t ds = mcpx_theta_shared_dim(d->family, d->n, d->m);
  // every group's sum starts from +0.0 and 0: empty groups keep them, the folds go on from them
  HIP_TRY(mcpx::launch_grouped_reduce_zero(c.dshared, c.dshared_ld, ds, g.G, c.used, st));
  if (d->batch == 0) return MCPX_OK;
  GroupTable t;
  build_groups(d, g.shared, g.shared_ld, g.G, g.off, ds, false, true, &t);
  DevGroups dg;
  HIP_TRY(dg.upload(t, st));
  a.group_map = dg.map;
  a.shared_ld = g.shared_ld;
  if (!a.x) a.x = a.theta;
  if (!a.y) a.y = a.theta;
  if (!a.s) a.s = a.theta;
  return launch_grouped_reduce(d, a, plan, c.skip, t, dg.chunks, dg.cbase, 0, (int64_t)t.chunks.size(), 0, c.dshared,
                               c.dshared_ld, c.used, nullptr, nullptr, st);
}

// One device's share of the host call: the chunks [cs, ce) of the table and their instances.
int grouped_reduce_shard(int dev, const mcpx_desc* d, const mcpx::SensArgs& a, const SensPlan& plan,
                         const GroupReduceCall& c, const GroupTable& t, double* hpart, int64_t* hcount, int64_t cs,
                         int64_t ce) {
  HIP_TRY(hipSetDevice(dev));
  int rc = check_device(dev);
  if (rc) return rc;
  const int n = d->n, m = d->m;
  const int64_t ds = mcpx_theta_shared_dim(d->family, n, m), nsh = t.G * ds;
  const int64_t b0 = t.chunks[(size_t)cs].first;
  const int64_t nb = t.chunks[(size_t)ce - 1].first + t.chunks[(size_t)ce - 1].len - b0;
  DevBuf<double> th, dx, dy, dsl, dgx, dgy, dgs, dout;
  DevBuf<int32_t> dst, dmap;
  DevBuf<uint8_t> dskip;
  DevBuf<mcpx::GroupChunk> dch;
  auto up = [&](DevBuf<double>& b, const double* h, size_t per) -> hipError_t {
    if (!h || !per) return hipSuccess;
    hipError_t e = b.alloc((size_t)nb * per);
    return e != hipSuccess ? e : hipMemcpy(b.p, h + b0 * per, sizeof(double) * nb * per, hipMemcpyHostToDevice);
  };
  HIP_TRY(th.alloc((size_t)std::max<int64_t>(nsh, 1)));
  if (nsh > 0) HIP_TRY(hipMemcpy(th.p, a.theta, sizeof(double) * (size_t)nsh, hipMemcpyHostToDevice));
  HIP_TRY(up(dx, a.x, n)); HIP_TRY(up(dy, a.y, m)); HIP_TRY(up(dsl, a.s, m));
  HIP_TRY(up(dgx, a.gx, n)); HIP_TRY(up(dgy, a.gy, m)); HIP_TRY(up(dgs, a.gs, m));
  if (c.skip) {
    HIP_TRY(dskip.alloc((size_t)nb));
    HIP_TRY(hipMemcpy(dskip.p, c.skip + b0, (size_t)nb, hipMemcpyHostToDevice));
  }
  HIP_TRY(dmap.alloc((size_t)nb));
  HIP_TRY(hipMemcpy(dmap.p, t.map.data() + b0, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice));
  HIP_TRY(dch.alloc((size_t)(ce - cs)));
  HIP_TRY(hipMemcpy(dch.p, t.chunks.data() + cs, sizeof(mcpx::GroupChunk) * (size_t)(ce - cs), hipMemcpyHostToDevice));
  if (a.out) HIP_TRY(dout.alloc((size_t)nb * (n + m)));
  if (a.status) HIP_TRY(dst.alloc((size_t)nb));
  mcpx_desc dd = *d;
  dd.batch = nb;
  mcpx::SensArgs da = a;  // the same call on the shard's device buffers
  da.theta = th.p;
  da.x = dx.p ? dx.p : th.p;
  da.y = dy.p ? dy.p : th.p;
  da.s = dsl.p ? dsl.p : th.p;
  da.gx = dgx.p;
  da.gy = dgy.p;
  da.gs = dgs.p;
  da.out = dout.p;
  da.status = dst.p;
  da.group_map = dmap.p;
  da.shared_ld = ds;
  rc = launch_grouped_reduce(&dd, da, plan, dskip.p, t, dch.p, nullptr, cs, ce, b0, nullptr, 0, nullptr, hpart, hcount,
                             nullptr);
  if (rc) {
    (void)hipDeviceSynchronize();  // nothing may still run on the buffers freed on return
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (a.out) HIP_TRY(hipMemcpy(a.out + b0 * (n + m), dout.p, sizeof(double) * nb * (n + m), hipMemcpyDeviceToHost));
  if (a.status) HIP_TRY(hipMemcpy(a.status + b0, dst.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
  return MCPX_OK;
}

int grouped_reduce_host(const mcpx_desc* d, const GroupCall& g, mcpx::SensArgs a, const GroupReduceCall& c,
                        int num_devices) {
  SensPlan plan;
  int rc;
  if ((rc = grouped_reduce_checks(d, g, c, &a, &plan))) return rc;
  const int64_t ds = mcpx_theta_shared_dim(d->family, d->n, d->m);
  for (int32_t k = 0; k < g.G; ++k) {  // the empty sums
    std::fill(c.dshared + k * c.dshared_ld, c.dshared + k * c.dshared_ld + ds, 0.0);
    c.used[k] = 0;
  }
  if (d->batch == 0) return MCPX_OK;
  if (mcpx_device_count() < 1) return fail(MCPX_ENODEV, "no HIP device visible");
  GroupTable t;
  build_groups(d, g.shared, g.shared_ld, g.G, g.off, ds, true, true, &t);
  if (!t.packed.empty()) a.theta = t.packed.data();
  const int64_t nch = (int64_t)t.chunks.size();
  std::vector<double> hpart((size_t)(nch * ds));
  std::vector<int64_t> hcount((size_t)nch, 0);
  // shards are runs of whole chunks of the table: a shard may cut a group, never a chunk
  rc = run_shards(num_devices, nch, [&](int dev, int64_t cs, int64_t ncs) {
    return grouped_reduce_shard(dev, d, a, plan, c, t, hpart.data(), hcount.data(), cs, cs + ncs);
  });
  if (rc) return rc;
  for (int32_t k = 0; k < g.G; ++k) {  // each group's chunk partials in its chunk order (grouped_reduce_fold)
    double* out = c.dshared + k * c.dshared_ld;
    for (int64_t q = t.cbase[(size_t)k]; q < t.cbase[(size_t)k + 1]; ++q) {
      const double* p = hpart.data() + q * ds;
      for (int64_t e = 0; e < ds; ++e) out[e] = out[e] + p[e];
      c.used[k] += hcount[(size_t)q];
    }
  }
  return MCPX_OK;
}

}  // namespace

extern "C" {

int mcpx_version(void) { return MCPX_VERSION; }

const char* mcpx_last_error(void) { return g_err.c_str(); }

void mcpx_default_params(mcpx_params* p) {
  if (!p) return;
  p->tol = 1e-4;              // src/solver.jl:42
  p->max_inner_iters = 20;    // :43
  p->max_outer_iters = 50;    // :44
  p->tightening_rate = 0.1;   // :45
  p->loosening_rate = 0.5;    // :46
  p->min_stepsize = 1e-4;     // :48
  p->tau = 0.995;             // :127
  p->decay = 0.5;             // :127
  p->linear_solver = MCPX_LINSOLVE_REDUCED;
  p->kernel = MCPX_KERNEL_AUTO;
}

int64_t mcpx_theta_dim(int32_t family, int32_t n, int32_t m) {
  if (n < 0 || m < 0) return -1;
  if (family == MCPX_FAMILY_QP) return (int64_t)n * n + (int64_t)m * n + m + n;
  if (family == MCPX_FAMILY_AFFINE) return (int64_t)n * n + 2 * (int64_t)n * m + (int64_t)m * m + n + m;
  return -1;
}

int64_t mcpx_theta_shared_dim(int32_t family, int32_t n, int32_t m) {
  if (n < 0 || m < 0) return -1;
  if (family == MCPX_FAMILY_QP) return (int64_t)n * n + (int64_t)m * n;
  if (family == MCPX_FAMILY_AFFINE) return (int64_t)n * n + 2 * (int64_t)n * m + (int64_t)m * m;
  return -1;
}

int64_t mcpx_theta_var_dim(int32_t family, int32_t n, int32_t m) {
  if (n < 0 || m < 0) return -1;
  if (family == MCPX_FAMILY_QP || family == MCPX_FAMILY_AFFINE) return (int64_t)n + m;
  return -1;
}

int mcpx_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int64_t mcpx_debug_canary_violations(void) { return g_canary_bad.load(); }

int mcpx_solve_batch_device(const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
                            const double* s0, const mcpx_params* prm, const mcpx_out* o, void* stream) {
  return solve_device_impl(nullptr, d, theta, x0, y0, s0, prm, o, stream);
}

int mcpx_solve_vjp_batch_device(const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
                                const double* s0, const mcpx_params* prm, const mcpx_out* out,
                                const mcpx_cotangent* ct, double* dtheta, int32_t* vjp_status, void* stream) {
  return solve_vjp_device_impl(d, theta, x0, y0, s0, prm, out, ct, dtheta, vjp_status, stream);
}

int mcpx_solve_batch(const mcpx_desc* d, const double* theta, const double* x0, const double* y0,
                     const double* s0, const mcpx_params* prm, int num_devices, mcpx_out* o) {
  return solve_host_impl(nullptr, d, theta, x0, y0, s0, prm, num_devices, o);
}

int mcpx_solve_batch_shared_device(const mcpx_desc* d, const double* theta_shared, const double* theta_var,
                                   const double* x0, const double* y0, const double* s0, const mcpx_params* prm,
                                   const mcpx_out* o, void* stream) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  bool empty = false;
  int rc = prepare_shared(d, theta_shared, theta_var, prm, o, &a, &plan, &empty);
  if (rc || empty) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  return launch_shared_chunks(d, theta_shared, theta_var, x0, y0, s0, o, a, plan, (hipStream_t)stream);
}

int mcpx_solve_batch_shared(const mcpx_desc* d, const double* theta_shared, const double* theta_var,
                            const double* x0, const double* y0, const double* s0, const mcpx_params* prm,
                            int num_devices, mcpx_out* o) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  bool empty = false;
  const int rc = prepare_shared(d, theta_shared, theta_var, prm, o, &a, &plan, &empty);
  if (rc || empty) return rc;
  return run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
    return solve_shard(dev, d, theta_shared, theta_var, x0, y0, s0, a, plan, o, b0, nb);
  });
}

int mcpx_solve_vjp_batch_shared_device(const mcpx_desc* d, const double* theta_shared, const double* theta_var,
                                       const double* x0, const double* y0, const double* s0,
                                       const mcpx_params* prm, const mcpx_out* out, const mcpx_cotangent* ct,
                                       double* dvar, int32_t* vjp_status, void* stream) {
  return solve_vjp_shared_device_impl(d, theta_shared, theta_var, x0, y0, s0, prm, out, ct, dvar, vjp_status,
                                      stream);
}

int mcpx_vjp_batch_shared_device(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                                 const double* s, const double* gx, const double* gy, const double* gs,
                                 double* dvar, int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_device(kVjp, nullptr, d, a, stream, true);
}

int mcpx_vjp_batch_shared(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                          const double* s, const double* gx, const double* gy, const double* gs, int num_devices,
                          double* dvar, int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_host(kVjp, nullptr, d, a, num_devices, true);
}

int mcpx_vjp_batch_shared_reduce_device(const mcpx_desc* d, const double* theta_shared, const double* x,
                                        const double* y, const double* s, const double* gx, const double* gy,
                                        const double* gs, const uint8_t* skip, double* dshared, int64_t* used,
                                        double* dvar, int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return shared_reduce_device(d, a, ReduceCall{skip, dshared, used}, stream);
}

int mcpx_vjp_batch_shared_reduce(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                                 const double* s, const double* gx, const double* gy, const double* gs,
                                 const uint8_t* skip, int num_devices, double* dshared, int64_t* used, double* dvar,
                                 int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return shared_reduce_host(d, a, ReduceCall{skip, dshared, used}, num_devices);
}

int mcpx_solve_batch_grouped_device(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld,
                                    int32_t num_groups, const int64_t* group_offsets, const double* theta_var,
                                    const double* x0, const double* y0, const double* s0, const mcpx_params* prm,
                                    const mcpx_out* o, void* stream) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  bool empty = false;
  const GroupCall g{theta_shared, shared_ld, num_groups, group_offsets};
  int rc = prepare_grouped(d, g, theta_var, prm, o, &a, &plan, &empty);
  if (rc || empty) return rc;
  int dev = 0;
  if ((rc = current_device(&dev))) return rc;
  const hipStream_t st = (hipStream_t)stream;
  GroupTable t;
  build_groups(d, theta_shared, shared_ld, num_groups, group_offsets, 0, false, false, &t);
  DevGroups dg;
  HIP_TRY(dg.upload(t, st));
  return launch_shared_chunks(d, theta_shared, theta_var, x0, y0, s0, o, a, plan, st, dg.map, shared_ld);
}

int mcpx_solve_batch_grouped(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld, int32_t num_groups,
                             const int64_t* group_offsets, const double* theta_var, const double* x0,
                             const double* y0, const double* s0, const mcpx_params* prm, int num_devices,
                             mcpx_out* o) {
  mcpx::KernelArgs a;
  SolvePlan plan;
  bool empty = false;
  const GroupCall g{theta_shared, shared_ld, num_groups, group_offsets};
  const int rc = prepare_grouped(d, g, theta_var, prm, o, &a, &plan, &empty);
  if (rc || empty) return rc;
  GroupTable t;
  build_groups(d, theta_shared, shared_ld, num_groups, group_offsets, mcpx_theta_shared_dim(d->family, d->n, d->m), true,
               false, &t);
  const double* blocks = t.packed.empty() ? theta_shared : t.packed.data();
  return run_shards(num_devices, d->batch, [&](int dev, int64_t b0, int64_t nb) {
    return solve_shard(dev, d, blocks, theta_var, x0, y0, s0, a, plan, o, b0, nb, &t);
  });
}

int mcpx_vjp_batch_grouped_device(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld,
                                  int32_t num_groups, const int64_t* group_offsets, const double* x, const double* y,
                                  const double* s, const double* gx, const double* gy, const double* gs,
                                  double* dvar, int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return grouped_vjp_device(d, GroupCall{theta_shared, shared_ld, num_groups, group_offsets}, a, stream);
}

int mcpx_vjp_batch_grouped(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld, int32_t num_groups,
                           const int64_t* group_offsets, const double* x, const double* y, const double* s,
                           const double* gx, const double* gy, const double* gs, int num_devices, double* dvar,
                           int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return grouped_vjp_host(d, GroupCall{theta_shared, shared_ld, num_groups, group_offsets}, a, num_devices);
}

int mcpx_vjp_batch_grouped_reduce_device(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld,
                                         int32_t num_groups, const int64_t* group_offsets, const double* x,
                                         const double* y, const double* s, const double* gx, const double* gy,
                                         const double* gs, const uint8_t* skip, double* dshared, int64_t dshared_ld,
                                         int64_t* used, double* dvar, int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return grouped_reduce_device(d, GroupCall{theta_shared, shared_ld, num_groups, group_offsets}, a,
                               GroupReduceCall{skip, dshared, dshared_ld, used}, stream);
}

int mcpx_vjp_batch_grouped_reduce(const mcpx_desc* d, const double* theta_shared, int64_t shared_ld,
                                  int32_t num_groups, const int64_t* group_offsets, const double* x, const double* y,
                                  const double* s, const double* gx, const double* gy, const double* gs,
                                  const uint8_t* skip, int num_devices, double* dshared, int64_t dshared_ld,
                                  int64_t* used, double* dvar, int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, dvar, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return grouped_reduce_host(d, GroupCall{theta_shared, shared_ld, num_groups, group_offsets}, a,
                             GroupReduceCall{skip, dshared, dshared_ld, used}, num_devices);
}

int mcpx_jvp_batch_shared_device(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                                 const double* s, int32_t n_partials, const double* var_dot, double* zdot,
                                 int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = var_dot;
  return sens_device(kJvp, nullptr, d, a, stream, true);
}

int mcpx_jvp_batch_shared(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                          const double* s, int32_t n_partials, const double* var_dot, int num_devices, double* zdot,
                          int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = var_dot;
  return sens_host(kJvp, nullptr, d, a, num_devices, true);
}

int mcpx_jvp_batch_shared_dot_device(const mcpx_desc* d, const double* theta_shared, const double* x,
                                     const double* y, const double* s, int32_t n_partials, const double* shared_dot,
                                     const double* var_dot, double* zdot, int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.shared_dot = shared_dot;
  a.theta_dot = var_dot;
  return sens_device(kJvp, nullptr, d, a, stream, true, true);
}

int mcpx_jvp_batch_shared_dot(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                              const double* s, int32_t n_partials, const double* shared_dot, const double* var_dot,
                              int num_devices, double* zdot, int32_t* status) {
  mcpx::SensArgs a = sens_args(theta_shared, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.shared_dot = shared_dot;
  a.theta_dot = var_dot;
  return sens_host(kJvp, nullptr, d, a, num_devices, true, true);
}

int mcpx_cond_batch_shared(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                           const double* s, int num_devices, double* rcond, int32_t* status) {
  return sens_host(kCond, nullptr, d, sens_args(theta_shared, x, y, s, rcond, status), num_devices, true);
}

int mcpx_cond_batch_shared_device(const mcpx_desc* d, const double* theta_shared, const double* x, const double* y,
                                  const double* s, double* rcond, int32_t* status, void* stream) {
  return sens_device(kCond, nullptr, d, sens_args(theta_shared, x, y, s, rcond, status), stream, true);
}

int mcpx_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(MCPX_EINVAL, "mcpx_host_register: NULL pointer or empty range");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
  return MCPX_OK;
}

int mcpx_host_unregister(void* ptr) {
  if (!ptr) return fail(MCPX_EINVAL, "mcpx_host_unregister: NULL pointer");
  HIP_TRY(hipHostUnregister(ptr));
  return MCPX_OK;
}

int mcpx_vjp_batch_device(const mcpx_desc* d, const double* theta, const double* x, const double* y,
                          const double* s, const double* gx, const double* gy, const double* gs, double* dtheta,
                          int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta, x, y, s, dtheta, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_device(kVjp, nullptr, d, a, stream);
}

int mcpx_vjp_batch(const mcpx_desc* d, const double* theta, const double* x, const double* y, const double* s,
                   const double* gx, const double* gy, const double* gs, int num_devices, double* dtheta,
                   int32_t* status) {
  mcpx::SensArgs a = sens_args(theta, x, y, s, dtheta, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_host(kVjp, nullptr, d, a, num_devices);
}

int mcpx_jvp_batch_device(const mcpx_desc* d, const double* theta, const double* x, const double* y,
                          const double* s, int32_t n_partials, const double* theta_dot, double* zdot,
                          int32_t* status, void* stream) {
  mcpx::SensArgs a = sens_args(theta, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = theta_dot;
  return sens_device(kJvp, nullptr, d, a, stream);
}

int mcpx_jvp_batch(const mcpx_desc* d, const double* theta, const double* x, const double* y, const double* s,
                   int32_t n_partials, const double* theta_dot, int num_devices, double* zdot, int32_t* status) {
  mcpx::SensArgs a = sens_args(theta, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = theta_dot;
  return sens_host(kJvp, nullptr, d, a, num_devices);
}

int mcpx_cond_batch(const mcpx_desc* d, const double* theta, const double* x, const double* y, const double* s,
                    int num_devices, double* rcond, int32_t* status) {
  return sens_host(kCond, nullptr, d, sens_args(theta, x, y, s, rcond, status), num_devices);
}

int mcpx_cond_batch_device(const mcpx_desc* d, const double* theta, const double* x, const double* y,
                           const double* s, double* rcond, int32_t* status, void* stream) {
  return sens_device(kCond, nullptr, d, sens_args(theta, x, y, s, rcond, status), stream);
}

int mcpx_cond_batch_module(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                           const double* y, const double* s, int num_devices, double* rcond, int32_t* status) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  return sens_host(kCond, mod, d, sens_args(theta, x, y, s, rcond, status), num_devices);
}

int mcpx_cond_batch_module_device(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                                  const double* y, const double* s, double* rcond, int32_t* status, void* stream) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  return sens_device(kCond, mod, d, sens_args(theta, x, y, s, rcond, status), stream);
}

int mcpx_vjp_batch_module(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                          const double* y, const double* s, const double* gx, const double* gy, const double* gs,
                          int num_devices, double* dtheta, int32_t* status) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  mcpx::SensArgs a = sens_args(theta, x, y, s, dtheta, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_host(kVjp, mod, d, a, num_devices);
}

int mcpx_vjp_batch_module_device(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                                 const double* y, const double* s, const double* gx, const double* gy,
                                 const double* gs, double* dtheta, int32_t* status, void* stream) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  mcpx::SensArgs a = sens_args(theta, x, y, s, dtheta, status);
  a.gx = gx;
  a.gy = gy;
  a.gs = gs;
  return sens_device(kVjp, mod, d, a, stream);
}

int mcpx_jvp_batch_module(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                          const double* y, const double* s, int32_t n_partials, const double* theta_dot,
                          int num_devices, double* zdot, int32_t* status) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  mcpx::SensArgs a = sens_args(theta, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = theta_dot;
  return sens_host(kJvp, mod, d, a, num_devices);
}

int mcpx_jvp_batch_module_device(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x,
                                 const double* y, const double* s, int32_t n_partials, const double* theta_dot,
                                 double* zdot, int32_t* status, void* stream) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  mcpx::SensArgs a = sens_args(theta, x, y, s, zdot, status);
  a.n_partials = n_partials;
  a.theta_dot = theta_dot;
  return sens_device(kJvp, mod, d, a, stream);
}

// ---- generated nonlinear modules (MCPX_FAMILY_NONLINEAR) ----------------------

int mcpx_solve_batch_module(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x0,
                            const double* y0, const double* s0, const mcpx_params* prm, int num_devices,
                            mcpx_out* o) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  return solve_host_impl(mod, d, theta, x0, y0, s0, prm, num_devices, o);
}

int mcpx_solve_batch_module_device(mcpx_module* mod, const mcpx_desc* d, const double* theta, const double* x0,
                                   const double* y0, const double* s0, const mcpx_params* prm,
                                   const mcpx_out* o, void* stream) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  return solve_device_impl(mod, d, theta, x0, y0, s0, prm, o, stream);
}

int mcpx_module_load(const char* path, mcpx_module** out) {
  if (!path || !out) return fail(MCPX_EINVAL, "path and out must be non-NULL");
  *out = nullptr;
  std::vector<char> img;
  {
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(MCPX_EINVAL, "cannot open code object '%s'", path);
    char buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) img.insert(img.end(), buf, buf + k);
    std::fclose(f);
  }
  if (img.empty()) return fail(MCPX_EINVAL, "code object '%s' is empty", path);
  if (mcpx_device_count() < 1) return fail(MCPX_ENODEV, "no HIP device visible");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  int rc = check_device(dev);
  if (rc) return rc;
  std::unique_ptr<mcpx_module> mod(new mcpx_module);
  mod->image = std::move(img);
  hipModule_t hm;
  if ((rc = module_on(mod.get(), dev, &hm))) return rc;
  hipDeviceptr_t dp = nullptr;
  size_t bytes = 0;
  if (hipModuleGetGlobal(&dp, &bytes, hm, "mcpx_nl_meta") != hipSuccess || bytes != sizeof mod->meta) {
    (void)hipModuleUnload(hm);
    return fail(MCPX_EINVAL, "'%s' is not an mcpx nonlinear module (no mcpx_nl_meta)", path);
  }
  HIP_TRY(hipMemcpyDtoH(mod->meta, dp, bytes));
  if (mod->meta[kMetaLayout] != kNLLayout) {
    (void)hipModuleUnload(hm);
    return fail(MCPX_EINVAL, "module layout version %d, this library expects %d", mod->meta[kMetaLayout], kNLLayout);
  }
  *out = mod.release();
  return MCPX_OK;
}

int mcpx_module_dims(const mcpx_module* mod, int32_t* n, int32_t* m, int32_t* p, int32_t* solvers) {
  if (!mod) return fail(MCPX_EINVAL, "module is NULL");
  if (n) *n = mod->meta[kMetaN];
  if (m) *m = mod->meta[kMetaM];
  if (p) *p = mod->meta[kMetaP];
  if (solvers) *solvers = mod->meta[kMetaKernels];
  return MCPX_OK;
}

void mcpx_module_unload(mcpx_module* mod) {
  if (!mod) return;
  int prev = 0;
  const bool have = hipGetDevice(&prev) == hipSuccess;
  for (auto& kv : mod->loaded)
    if (hipSetDevice(kv.first) == hipSuccess) (void)hipModuleUnload(kv.second);
  if (have) (void)hipSetDevice(prev);
  delete mod;
}

}  // extern "C"
