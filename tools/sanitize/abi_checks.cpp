// Host-side sanitizer driver (SURVEY.md §5 "Race detection / sanitizers"): the C
// ABI's host code (mcpx_api.cpp, compiled with -fsanitize=address,undefined on
// the host side only) exercised through every argument-checking and no-device
// path, from several threads at once (the thread-local error string, the
// reentrancy claim of include/mcpx.h).  Built and run by tools/sanitize/run.sh;
// needs no GPU (without one every compute call must return MCPX_ENODEV).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/mcpx.h"
#include "../../mcp_amd/csrc/wg_layout.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static void one_thread(int seed) {
  const bool gpu = mcpx_device_count() > 0;
  mcpx_params p;
  std::memset(&p, 0xAB, sizeof p);  // garbage first: mcpx_default_params must set every field
  mcpx_default_params(&p);
  EXPECT(p.tol == 1e-4 && p.max_inner_iters == 20 && p.max_outer_iters == 50 && p.kernel == MCPX_KERNEL_AUTO);
  EXPECT(p.linear_solver == MCPX_LINSOLVE_REDUCED);
  const int n = 3 + seed % 5, m = 2 + seed % 3;
  const int64_t pdim = mcpx_theta_dim(MCPX_FAMILY_QP, n, m);
  EXPECT(pdim == (int64_t)n * n + m * n + m + n);
  EXPECT(mcpx_theta_dim(7, n, m) < 0 && mcpx_theta_dim(MCPX_FAMILY_QP, -1, m) < 0);
  const int B = 4;
  std::vector<double> theta(B * pdim, 0.5), x(B * n), y(B * m), s(B * m), kkt(B), eps(B);
  std::vector<int32_t> outer(B), status(B), newton(B);
  mcpx_out o{};
  o.x = x.data(); o.y = y.data(); o.s = s.data(); o.kkt_error = kkt.data(); o.eps = eps.data();
  o.outer_iters = outer.data(); o.status = status.data(); o.newton_iters = newton.data();
  mcpx_desc d{MCPX_FAMILY_QP, n, m, 0, B, pdim};
  // argument errors: never touch the buffers, always leave a message
  mcpx_desc bad = d;
  bad.theta_ld = pdim - 1;
  EXPECT(mcpx_solve_batch(&bad, theta.data(), nullptr, nullptr, nullptr, &p, 1, &o) == MCPX_EINVAL);
  EXPECT(std::strlen(mcpx_last_error()) > 0);
  bad = d;
  bad.batch = -1;
  EXPECT(mcpx_solve_batch(&bad, theta.data(), nullptr, nullptr, nullptr, &p, 1, &o) == MCPX_EINVAL);
  EXPECT(mcpx_solve_batch(nullptr, theta.data(), nullptr, nullptr, nullptr, &p, 1, &o) == MCPX_EINVAL);
  EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, nullptr, 1, &o) == MCPX_EINVAL);
  mcpx_params q = p;
  q.kernel = 9;
  EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, &q, 1, &o) == MCPX_EINVAL);
  q = p;
  q.decay = std::nan("");
  EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, &q, 1, &o) == MCPX_EINVAL);
  q = p;
  q.max_inner_iters = 100000;
  EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, &q, 1, &o) == MCPX_EUNSUPPORTED);
  q = p;
  q.linear_solver = MCPX_LINSOLVE_SCHUR;
  mcpx_desc big{MCPX_FAMILY_QP, 130, 20, 0, 1, mcpx_theta_dim(MCPX_FAMILY_QP, 130, 20)};  // QP SCHUR: n ≤ 128
  EXPECT(mcpx_solve_batch(&big, theta.data(), nullptr, nullptr, nullptr, &q, 1, &o) == MCPX_EUNSUPPORTED);
  mcpx_out none{};
  EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, &p, 1, &none) == MCPX_EINVAL);
  // sensitivities: argument checks
  std::vector<double> dth(B * pdim);
  EXPECT(mcpx_vjp_batch(&d, nullptr, x.data(), y.data(), s.data(), nullptr, nullptr, nullptr, 1, dth.data(),
                        nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_jvp_batch(&d, theta.data(), x.data(), y.data(), s.data(), -1, nullptr, 1, dth.data(), nullptr) ==
         MCPX_EINVAL);
  // module loading: missing / empty / foreign files
  mcpx_module* mod = nullptr;
  EXPECT(mcpx_module_load("/nonexistent/file.hsaco", &mod) == MCPX_EINVAL && mod == nullptr);
  EXPECT(mcpx_module_load(nullptr, &mod) == MCPX_EINVAL);
  EXPECT(mcpx_module_dims(nullptr, nullptr, nullptr, nullptr, nullptr) == MCPX_EINVAL);
  mcpx_module_unload(nullptr);
  if (!gpu) {  // a valid call without a device: an error, never a CPU fallback
    EXPECT(mcpx_solve_batch(&d, theta.data(), nullptr, nullptr, nullptr, &p, 1, &o) == MCPX_ENODEV);
    EXPECT(mcpx_vjp_batch(&d, theta.data(), x.data(), y.data(), s.data(), nullptr, nullptr, nullptr, 1,
                          dth.data(), nullptr) == MCPX_ENODEV);
  }
}

// Every failure of the descriptor / parameter validation (prepare, prepare_sens of
// mcpx_api.cpp) returns its code through each entry point that reaches it, and the
// checks keep their precedence.  No call here gets as far as a device.
struct Bufs {
  std::vector<double> theta, x, y, s, out;
  std::vector<int32_t> i32;
  mcpx_out o{};
  mcpx_cotangent ct{};
  explicit Bufs(size_t k) : theta(k, 0.5), x(k), y(k), s(k), out(k), i32(k) {
    o.x = x.data(); o.y = y.data(); o.s = s.data(); o.kkt_error = out.data(); o.eps = out.data();
    o.outer_iters = i32.data(); o.status = i32.data();
  }
};
using SolveFn = int (*)(const mcpx_desc*, const mcpx_params*, Bufs&);
using SensFn = int (*)(const mcpx_desc*, Bufs&);

static const SolveFn kSolve[] = {
    [](const mcpx_desc* d, const mcpx_params* p, Bufs& b) {
      return mcpx_solve_batch(d, b.theta.data(), nullptr, nullptr, nullptr, p, 1, &b.o);
    },
    [](const mcpx_desc* d, const mcpx_params* p, Bufs& b) {
      return mcpx_solve_batch_device(d, b.theta.data(), nullptr, nullptr, nullptr, p, &b.o, nullptr);
    },
    [](const mcpx_desc* d, const mcpx_params* p, Bufs& b) {
      return mcpx_solve_vjp_batch_device(d, b.theta.data(), nullptr, nullptr, nullptr, p, &b.o, &b.ct, b.out.data(),
                                         nullptr, nullptr);
    },
};
static const SensFn kSens[] = {
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_vjp_batch(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), nullptr, nullptr, nullptr, 1,
                            b.out.data(), nullptr);
    },
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_vjp_batch_device(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), nullptr, nullptr, nullptr,
                                   b.out.data(), nullptr, nullptr);
    },
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_jvp_batch(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), 1, b.theta.data(), 1,
                            b.out.data(), nullptr);
    },
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_jvp_batch_device(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), 1, b.theta.data(),
                                   b.out.data(), nullptr, nullptr);
    },
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_cond_batch(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), 1, b.out.data(), nullptr);
    },
    [](const mcpx_desc* d, Bufs& b) {
      return mcpx_cond_batch_device(d, b.theta.data(), b.x.data(), b.y.data(), b.s.data(), b.out.data(), nullptr,
                                    nullptr);
    },
};

static bool last_error_has(const char* text) { return std::strstr(mcpx_last_error(), text) != nullptr; }

static void validation_checks() {
  const bool gpu = mcpx_device_count() > 0;
  const int n = 4, m = 3;
  const int64_t pdim = mcpx_theta_dim(MCPX_FAMILY_QP, n, m);
  Bufs b(4 * (size_t)pdim);
  mcpx_params p;
  mcpx_default_params(&p);
  const mcpx_desc good{MCPX_FAMILY_QP, n, m, 0, 4, pdim};

  // descriptor failures: the same code from the solves and from the sensitivities
  struct DescCase { mcpx_desc d; int code; const char* text; };
  auto with = [&](auto&& edit) { mcpx_desc d = good; edit(d); return d; };
  const DescCase desc_cases[] = {
      {with([](mcpx_desc& d) { d.family = MCPX_FAMILY_NONLINEAR; }), MCPX_EINVAL, "generated module"},
      {with([](mcpx_desc& d) { d.family = 7; }), MCPX_EINVAL, "bad family"},
      {with([](mcpx_desc& d) { d.n = -1; }), MCPX_EINVAL, "negative dimensions"},
      {with([](mcpx_desc& d) { d.n = 0; d.m = 0; }), MCPX_EINVAL, "empty problem"},
      {with([](mcpx_desc& d) { d.batch = -1; }), MCPX_EINVAL, "negative batch"},
      {with([](mcpx_desc& d) { d.theta_ld -= 1; }), MCPX_EINVAL, "theta_ld"},
      // n + 2m = 780 > MCPX_MAX_WG_KKT_DIM: beyond every kernel
      {with([](mcpx_desc& d) { d.n = 700; d.m = 40; d.theta_ld = mcpx_theta_dim(d.family, 700, 40); }),
       MCPX_EUNSUPPORTED, "n=700 m=40"},
  };
  for (const DescCase& c : desc_cases) {
    for (SolveFn f : kSolve) EXPECT(f(&c.d, &p, b) == c.code && last_error_has(c.text));
    for (SensFn f : kSens) EXPECT(f(&c.d, b) == c.code && last_error_has(c.text));
  }
  for (SolveFn f : kSolve) {
    EXPECT(f(nullptr, &p, b) == MCPX_EINVAL);
    EXPECT(f(&good, nullptr, b) == MCPX_EINVAL);
  }
  for (SensFn f : kSens) EXPECT(f(nullptr, b) == MCPX_EINVAL);

  // parameter failures of the solves
  struct ParamCase { mcpx_params p; int code; const char* text; };
  auto prm = [&](auto&& edit) { mcpx_params q = p; edit(q); return q; };
  const double nan = std::nan("");
  const ParamCase param_cases[] = {
      {prm([](mcpx_params& q) { q.linear_solver = 3; }), MCPX_EINVAL, "unknown linear_solver"},
      {prm([](mcpx_params& q) { q.linear_solver = -1; }), MCPX_EINVAL, "unknown linear_solver"},
      {prm([](mcpx_params& q) { q.kernel = 5; }), MCPX_EINVAL, "unknown kernel selector"},
      {prm([](mcpx_params& q) { q.kernel = -1; }), MCPX_EINVAL, "unknown kernel selector"},
      {prm([](mcpx_params& q) { q.kernel = MCPX_KERNEL_MULTIWAVE; }), MCPX_EUNSUPPORTED, "MCPX_KERNEL_MULTIWAVE"},
      {prm([](mcpx_params& q) { q.kernel = MCPX_KERNEL_BAND; }), MCPX_EUNSUPPORTED, "MCPX_KERNEL_BAND"},
      {prm([](mcpx_params& q) { q.tol = 0; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([&](mcpx_params& q) { q.tol = nan; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.min_stepsize = 0; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.decay = 0; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.decay = 1; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([&](mcpx_params& q) { q.tau = nan; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([&](mcpx_params& q) { q.tightening_rate = nan; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([&](mcpx_params& q) { q.loosening_rate = nan; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.max_inner_iters = 0; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.max_outer_iters = 0; }), MCPX_EINVAL, "invalid solver parameters"},
      {prm([](mcpx_params& q) { q.max_inner_iters = MCPX_MAX_INNER_ITERS + 1; }), MCPX_EUNSUPPORTED, "max_inner_iters"},
      // decay 0.5 down to 1e-30: 100 trials > MCPX_MAX_LS_TRIALS
      {prm([](mcpx_params& q) { q.min_stepsize = 1e-30; }), MCPX_EUNSUPPORTED, "line-search trials"},
  };
  for (const ParamCase& c : param_cases)
    for (SolveFn f : kSolve) EXPECT(f(&good, &c.p, b) == c.code && last_error_has(c.text));

  // sizes and selectors the kernels do not cover
  const mcpx_desc wide{MCPX_FAMILY_QP, 50, 20, 0, 4, mcpx_theta_dim(MCPX_FAMILY_QP, 50, 20)};      // n + m > 64
  const mcpx_desc tall{MCPX_FAMILY_QP, 130, 20, 0, 4, mcpx_theta_dim(MCPX_FAMILY_QP, 130, 20)};    // QP SCHUR: n <= 128
  const mcpx_desc aff{MCPX_FAMILY_AFFINE, n, m, 0, 4, mcpx_theta_dim(MCPX_FAMILY_AFFINE, n, m)};  // no workgroup SCHUR
  mcpx_params q = p;
  q.kernel = MCPX_KERNEL_WAVE;
  for (SolveFn f : kSolve) EXPECT(f(&wide, &q, b) == MCPX_EUNSUPPORTED && last_error_has("exceeds the kernels"));
  q = p;
  q.linear_solver = MCPX_LINSOLVE_SCHUR;
  for (SolveFn f : kSolve) EXPECT(f(&tall, &q, b) == MCPX_EUNSUPPORTED && last_error_has("exceeds the kernels"));
  q.kernel = MCPX_KERNEL_WORKGROUP;
  for (SolveFn f : kSolve) EXPECT(f(&aff, &q, b) == MCPX_EUNSUPPORTED && last_error_has("exceeds the kernels"));

  // precedence: a descriptor error wins over a bad solver selector, a bad selector over bad tolerances
  mcpx_desc bad = good;
  bad.theta_ld = pdim - 1;
  for (SolveFn f : kSolve) {
    q = p;
    q.linear_solver = 9;
    EXPECT(f(&bad, &q, b) == MCPX_EINVAL && last_error_has("theta_ld"));
    q = p;
    q.kernel = MCPX_KERNEL_MULTIWAVE;  // MCPX_EUNSUPPORTED on its own
    EXPECT(f(&bad, &q, b) == MCPX_EINVAL && last_error_has("theta_ld"));
    q.tol = -1;
    EXPECT(f(&good, &q, b) == MCPX_EUNSUPPORTED && last_error_has("MCPX_KERNEL_MULTIWAVE"));
    q = p;
    q.linear_solver = 9;
    q.tol = -1;
    EXPECT(f(&good, &q, b) == MCPX_EINVAL && last_error_has("unknown linear_solver"));
    q = p;
    q.kernel = 9;
    q.max_inner_iters = MCPX_MAX_INNER_ITERS + 1;  // MCPX_EUNSUPPORTED on its own
    EXPECT(f(&good, &q, b) == MCPX_EINVAL && last_error_has("unknown kernel selector"));
  }

  // what follows the validation: argument checks, the empty batch, and then the device
  mcpx_out none{};
  EXPECT(mcpx_solve_batch_device(&good, b.theta.data(), nullptr, nullptr, nullptr, &p, &none, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_solve_vjp_batch_device(&good, b.theta.data(), nullptr, nullptr, nullptr, &p, &none, &b.ct, b.out.data(),
                                     nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_solve_vjp_batch_device(&good, b.theta.data(), nullptr, nullptr, nullptr, &p, &b.o, nullptr, b.out.data(),
                                     nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_solve_vjp_batch_device(&good, b.theta.data(), nullptr, nullptr, nullptr, &p, &b.o, &b.ct, nullptr,
                                     nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_solve_batch_device(&good, nullptr, nullptr, nullptr, nullptr, &p, &b.o, nullptr) == MCPX_EINVAL);
  double *th = b.theta.data(), *x = b.x.data(), *y = b.y.data(), *s = b.s.data(), *out = b.out.data();
  EXPECT(mcpx_vjp_batch_device(&good, nullptr, x, y, s, nullptr, nullptr, nullptr, out, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_vjp_batch_device(&good, th, x, y, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_vjp_batch_device(&good, th, nullptr, y, s, nullptr, nullptr, nullptr, out, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_vjp_batch(&good, th, x, nullptr, s, nullptr, nullptr, nullptr, 1, out, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_cond_batch(&good, th, x, y, nullptr, 1, out, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_cond_batch_device(&good, th, x, y, s, nullptr, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_jvp_batch_device(&good, th, x, y, s, -1, th, out, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_jvp_batch_device(&good, th, x, y, s, 2, nullptr, out, nullptr, nullptr) == MCPX_EINVAL &&
         last_error_has("theta_dot"));
  EXPECT(mcpx_jvp_batch(&good, th, x, y, s, 2, nullptr, 1, out, nullptr) == MCPX_EINVAL && last_error_has("theta_dot"));
  EXPECT(mcpx_jvp_batch(&good, nullptr, x, y, s, 2, nullptr, 1, out, nullptr) == MCPX_EINVAL && !last_error_has("theta_dot"));
  mcpx_desc empty = good;
  empty.batch = 0;  // nothing to do: MCPX_OK before any pointer or device is looked at
  EXPECT(mcpx_solve_batch(&empty, nullptr, nullptr, nullptr, nullptr, &p, 1, &b.o) == MCPX_OK);
  EXPECT(mcpx_solve_batch_device(&empty, nullptr, nullptr, nullptr, nullptr, &p, &b.o, nullptr) == MCPX_OK);
  EXPECT(mcpx_solve_batch(&empty, nullptr, nullptr, nullptr, nullptr, &p, 1, &none) == MCPX_EINVAL);
  EXPECT(mcpx_solve_vjp_batch_device(&empty, nullptr, nullptr, nullptr, nullptr, &p, &b.o, &b.ct, nullptr, nullptr,
                                     nullptr) == MCPX_OK);
  EXPECT(mcpx_vjp_batch(&empty, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr) == MCPX_OK);
  EXPECT(mcpx_vjp_batch_device(&empty, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr) == MCPX_OK);
  EXPECT(mcpx_jvp_batch(&empty, nullptr, nullptr, nullptr, nullptr, 2, nullptr, 1, nullptr, nullptr) == MCPX_OK);
  EXPECT(mcpx_jvp_batch_device(&empty, nullptr, nullptr, nullptr, nullptr, 2, nullptr, nullptr, nullptr, nullptr) == MCPX_OK);
  EXPECT(mcpx_jvp_batch(&empty, nullptr, nullptr, nullptr, nullptr, -1, nullptr, 1, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_cond_batch(&empty, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr) == MCPX_OK);
  EXPECT(mcpx_cond_batch_device(&empty, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MCPX_OK);
  if (!gpu) {
    for (SolveFn f : kSolve) EXPECT(f(&good, &p, b) == MCPX_ENODEV);
    for (SensFn f : kSens) EXPECT(f(&good, b) == MCPX_ENODEV);
  }

  // module entry points: a NULL module is refused before anything else is looked at
  mcpx_desc nl = good;
  nl.family = MCPX_FAMILY_NONLINEAR;
  EXPECT(mcpx_solve_batch_module(nullptr, &nl, th, nullptr, nullptr, nullptr, &p, 1, &b.o) == MCPX_EINVAL);
  EXPECT(mcpx_solve_batch_module_device(nullptr, &nl, th, nullptr, nullptr, nullptr, &p, &b.o, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_vjp_batch_module(nullptr, &nl, th, x, y, s, nullptr, nullptr, nullptr, 1, out, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_vjp_batch_module_device(nullptr, &nl, th, x, y, s, nullptr, nullptr, nullptr, out, nullptr, nullptr) ==
         MCPX_EINVAL);
  EXPECT(mcpx_jvp_batch_module(nullptr, &nl, th, x, y, s, 1, th, 1, out, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_jvp_batch_module_device(nullptr, &nl, th, x, y, s, 1, th, out, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_cond_batch_module(nullptr, &nl, th, x, y, s, 1, out, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_cond_batch_module_device(nullptr, &nl, th, x, y, s, out, nullptr, nullptr) == MCPX_EINVAL);
  EXPECT(mcpx_solve_batch_module(nullptr, nullptr, th, nullptr, nullptr, nullptr, &p, 1, &b.o) == MCPX_EINVAL &&
         last_error_has("module is NULL"));
}

// The slot layouts and grid sizes of the persistent workgroup kernels (csrc/wg_layout.h):
// 256-B-aligned parts, MCPX_JVP_RHS partials per factorisation, the 4 GiB workspace cap.
static void layout_checks() {
  using namespace mcpx::wg;
  struct Solve { int n, m, solver; int64_t block; int ld; int64_t off_blk, off_aux, stride; };
  const Solve solve[] = {
      {128, 64, MCPX_LINSOLVE_SCHUR, 0, 129, 16512, 16512, 16768},
      {100, 150, MCPX_LINSOLVE_REDUCED, 0, 251, 62752, 62752, 62752},
      {40, 30, MCPX_LINSOLVE_DENSE, 0, 101, 10112, 10112, 10112},
      {37, 21, MCPX_LINSOLVE_SCHUR, 1234, 38, 1408, 2656, 2752},
  };
  for (const Solve& c : solve) {
    const WgArgs w = solve_layout(c.solver, c.n, c.m, c.block);
    EXPECT(w.ld == c.ld && w.off_blk == c.off_blk && w.off_aux == c.off_aux && w.slot_stride == c.stride);
    EXPECT(w.off_rd == w.off_aux);
    EXPECT(w.work == nullptr && w.counter == nullptr && w.batch == 0);  // the launch's part stays empty
  }
  struct Sens { bool jvp; int mode, n, m, K; int64_t p, block; int nrhs, ld; int64_t off_blk, off_dth, off_sol, stride; };
  const int64_t p_qp = mcpx_theta_dim(MCPX_FAMILY_QP, 100, 150);
  const Sens sens[] = {
      {true, 0, 100, 150, 11, p_qp, kNoModule, 8, 408, 163200, 163200, 163200, 166400},
      {true, 0, 37, 21, 3, 50, 1234, 3, 82, 6496, 7744, 10656, 10912},
      {false, 0, 100, 150, 0, p_qp, kNoModule, 1, 251, 62752, 62752, 62752, 62752},
      {false, 0, 37, 21, 0, 50, 1234, 1, 59, 3424, 4672, 7584, 7584},
      {true, 1, 37, 21, 0, 50, 1234, 2, 81, 6400, 7648, 10560, 10720},
  };
  for (const Sens& c : sens) {
    const WgSensArgs w = sens_layout(c.jvp, c.mode, c.n, c.m, c.p, c.K, c.block);
    EXPECT(w.nrhs == c.nrhs && w.ld == c.ld && w.off_blk == c.off_blk && w.off_dth == c.off_dth);
    EXPECT(w.off_sol == c.off_sol && w.slot_stride == c.stride);
  }
  EXPECT(sens_layout(true, 0, 37, 21, 50, 0, 1234).nrhs == 1);  // no partials: still one column
  EXPECT(grid_size(512, 1000, 4400000, kSensWorkCap) == 122);
  EXPECT(grid_size(512, 1000, 4400000, 0) == 512);
  EXPECT(grid_size(512, 3, 4400000, kSensWorkCap) == 3);
  EXPECT(grid_size(512, 1000, (int64_t)1 << 30, kSensWorkCap) == 1);  // a slot beyond the cap: one workgroup
  EXPECT(grid_size(512, kChunk + 5, 32, 0) == 512 && grid_size(2 * kChunk, 2 * kChunk, 0, 0) == kChunk);
}

int main() {
  EXPECT(mcpx_version() == MCPX_VERSION);
  validation_checks();
  layout_checks();
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t) ts.emplace_back(one_thread, t);
  for (auto& t : ts) t.join();
  std::printf("abi_checks: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
  return failures ? 1 : 0;
}
