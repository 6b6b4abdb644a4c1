// hd_api.cpp -- C-ABI of libhdisort.so (include/hdisort.h): argument
// validation, quadrature constants, scratch management, chunked launches,
// per-solve status, optional per-kernel timing with HIP events.
//
// Replaces pydisort's DisortImpl::forward batch loop over (nwave, ncol)
// [EXTERNAL, pydisort @ afee3ec897f] and its per-column c_disort calls
// (legacy: src/rtsolver/rt_solver_disort.cpp_:147,234; error behaviour:
// nonzero c_disort -> "DisortWrapper::Run failed.", :149-151).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hdbeer.h"
#include "../../include/hdharp.h"
#include "../../include/hdisort.h"
#include "hd_beer.hpp"
#include "hd_kernels.hpp"
#include "hd_team_prims.hpp"
#include "hd_rad.hpp"

struct hd_context {
  int device = 0;
  double* scratch = nullptr;
  size_t scratch_doubles = 0;
  // per-g fluxes of hd_solve_band's row-major route (band_rowmajor)
  double* pflux = nullptr;
  size_t pflux_doubles = 0;
  int band_cmaj = 0;  // A/B (HD_BAND_CMAJ=1): always the column-major fused epilogue
  int* status = nullptr;  // internal per-solve status (when caller passes NULL)
  size_t status_len = 0;
  int* anyerr = nullptr;
  long chunk = 0;  // 0 = auto
  bool timing = false;
  // timing: one event triple per launched chunk, resolved lazily in get_timing
  std::vector<hipEvent_t> pool;
  size_t pool_used = 0;
  hd_timing times{};
  int max_sweeps = 16;  // Jacobi sweep cap (debug setter: hd_context_set_max_sweeps)
  // team-path Jacobi from the tabulated (ssa, chi_1) eigenvectors
  // (hd_kernels.hpp); HD_JACOBI_WARM=0 in the environment turns it off (A/B)
  int warm = 1;
  // nstr 4 / 8: the sweep in NN-lane teams (hd_sweep_quad_kernel) for chunks of at
  // most kQuadMaxSolves solves (-1, the default), always (1) or never (0): HD_SWEEP_QUAD
  int quad = -1;
  // true while a solve enqueues into a capturing stream: scratch may not grow then
  bool capturing = false;
  std::string err;
  std::mutex err_mu;  // guards err (hd_last_error reads it without the solve lock)
  // register path: back-substitution of chunk k on `side`, beside chunk k+1's
  // layer kernel (its 44-VGPR waves fit next to the layer kernel's on a SIMD)
  hipStream_t side = nullptr;
  // register path: chunk k+1's layer kernel on its own stream, beside chunk k's
  // sweep (it takes the SIMDs a partial sweep leaves idle)
  hipStream_t lay = nullptr;
  hipEvent_t ev_layer[2] = {nullptr, nullptr};
  hipEvent_t ev_sweep[2] = {nullptr, nullptr};
  hipEvent_t ev_back[2] = {nullptr, nullptr};
  hipEvent_t ev_pro[2] = {nullptr, nullptr};  // next chunk's prologue done (side stream)
  hipEvent_t ev_fork = nullptr;                // start of a solve on the caller's stream
  double* sink = nullptr;                      // team kernels: stores of lanes >= nstr/2
  double* rad_grid = nullptr;                  // device copies of umu | phi | utau
  size_t rad_grid_len = 0;
  // Serialisation of the context's scratch (SURVEY 8(b) "Threading"): every
  // entry point holds `mu` while it enqueues, and every solve starts behind
  // `ev_done`, recorded on the caller's stream at the end of the previous
  // solve -- so two modules sharing this context from two streams (or two
  // host threads) never touch scratch/status/anyerr concurrently.
  std::mutex mu;
  hipEvent_t ev_done = nullptr;
  bool done_valid = false;
  // hd_solve_host / hd_solve_band_host: device copies of the caller's host arrays
  double* hstage = nullptr;
  size_t hstage_len = 0;  // doubles
  hipStream_t hstream = nullptr;   // host<->device copies
  hipStream_t hstream2 = nullptr;  // the pieces' solves
  hipStream_t hstream3 = nullptr;  // device->host copies (PCIe is full duplex: beside the uploads)
  hipEvent_t hev_in[2] = {nullptr, nullptr};
  hipEvent_t hev_done[2] = {nullptr, nullptr};
};

namespace {

std::mutex g_err_mu;
std::string g_err;

int fail(hd_context* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    ctx->err = buf;
  }
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = buf;
  return code;
}

#define HD_HIP(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(ctx, HD_EHIP, "%s failed: %s", #call, hipGetErrorString(e_));            \
  } while (0)

// Gauss-Legendre nodes/weights on (0,1), ascending (double-Gauss half range).
void gauss01(int nn, double* mu, double* w) {
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < (nn + 1) / 2; ++i) {
    double x = std::cos(pi * (i + 0.75) / (nn + 0.5));
    double dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = x;
      for (int l = 2; l <= nn; ++l) {
        double p2 = ((2 * l - 1) * x * p1 - (l - 1) * p0) / l;
        p0 = p1;
        p1 = p2;
      }
      dp = nn * (x * p1 - p0) / (x * x - 1.0);
      double dx = p1 / dp;
      x -= dx;
      if (std::fabs(dx) < 1e-16) break;
    }
    {
      double p0 = 1.0, p1 = x;
      for (int l = 2; l <= nn; ++l) {
        double p2 = ((2 * l - 1) * x * p1 - (l - 1) * p0) / l;
        p0 = p1;
        p1 = p2;
      }
      dp = nn * (x * p1 - p0) / (x * x - 1.0);
    }
    const double wx = 2.0 / ((1.0 - x * x) * dp * dp);
    mu[nn - 1 - i] = 0.5 * (1.0 + x);
    w[nn - 1 - i] = 0.5 * wx;
    mu[i] = 0.5 * (1.0 - x);
    w[i] = 0.5 * wx;
  }
}

void make_quad(int nn, hd::QuadHost& q) {
  std::memset(&q, 0, sizeof(q));
  gauss01(nn, q.mu, q.w);
  for (int i = 0; i < nn; ++i) {
    q.sd[i] = std::sqrt(q.w[i] / q.mu[i]);
    q.g[i] = std::sqrt(q.w[i] * q.mu[i]);
    double p0 = 1.0, p1 = q.mu[i];
    q.pt[0][i] = 1.0;
    if (2 * nn > 1) q.pt[1][i] = p1;
    for (int l = 2; l < 2 * nn; ++l) {
      double p2 = ((2 * l - 1) * q.mu[i] * p1 - (l - 1) * p0) / l;
      q.pt[l][i] = p2;
      p0 = p1;
      p1 = p2;
    }
  }
}

// The quadrature tables of every nn, built once per process; their upload into a
// device's __constant__ memory happens once per device (the module's constants
// are per device, shared by every context on it), under one global lock.
const hd::QuadHost* quad_host() {
  static hd::QuadHost all[hd::kMaxNN];
  static std::once_flag once;
  std::call_once(once, [] {
    for (int nn = 1; nn <= hd::kMaxNN; ++nn) make_quad(nn, all[nn - 1]);
  });
  return all;
}

constexpr int kMaxDevices = 64;
std::mutex g_tab_mu;
bool g_tables[kMaxDevices] = {};      // flux-path tables uploaded, per device
bool g_rad_tables[kMaxDevices] = {};  // intensity-path tables uploaded, per device

int ensure_tables(hd_context* ctx) {
  if (ctx->device < 0 || ctx->device >= kMaxDevices)
    return fail(ctx, HD_EINVAL, "hd_solve: device %d beyond the table cache", ctx->device);
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (g_tables[ctx->device]) return HD_OK;
  const hd::QuadHost* all = quad_host();
  hipError_t e = hd::upload_quad_tables(all);
  if (e == hipSuccess) e = hd::upload_quad_tables_team(all);
  if (e == hipSuccess) e = hd::upload_warm_tables_team(all);
  if (e != hipSuccess) return fail(ctx, HD_EHIP, "hd_solve: constant upload: %s", hipGetErrorString(e));
  g_tables[ctx->device] = true;
  return HD_OK;
}

int ensure_rad_tables(hd_context* ctx) {
  int rc = ensure_tables(ctx);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_tab_mu);
  if (g_rad_tables[ctx->device]) return HD_OK;
  hipError_t e = hd::upload_rad_tables(quad_host());
  if (e == hipSuccess) e = hd::upload_rad_tables_team(quad_host());
  if (e != hipSuccess)
    return fail(ctx, HD_EHIP, "hd_solve_radiance: constant upload: %s", hipGetErrorString(e));
  g_rad_tables[ctx->device] = true;
  return HD_OK;
}

using hd::auto_chunk;
using hd::max_auto_chunk;

// hd_solve_band's row-major route (hd_plan.hpp: band_rowmajor_size) under the context's
// switches
bool band_rowmajor(const hd_context* ctx, int nn, long nsolve) {
  return ctx->chunk <= 0 && !ctx->band_cmaj && hd::band_rowmajor_size(nn, nsolve);
}

// the last solve that used the context's buffers has finished (before a free)
void drain(hd_context* ctx) {
  if (ctx->done_valid) (void)hipEventSynchronize(ctx->ev_done);
}

// The messages of one of the context's device buffers, printf formats over (entry
// point, bytes).  capture null: a buffer no capturing call reaches.
struct BufText {
  const char* capture;
  const char* nomem;
};
constexpr BufText kScratchText{
    "%s: scratch must grow to %zu bytes inside a stream capture; size the "
    "context first (hd_context_reserve, or one eager call of the same shape)",
    "%s: cannot allocate %zu bytes of scratch"};
constexpr BufText kPfluxText{
    "%s: the per-g flux buffer must grow to %zu bytes inside a stream "
    "capture; size the context first (hd_context_reserve, or one eager call of the "
    "same shape)",
    "%s: cannot allocate %zu bytes of per-g fluxes"};
constexpr BufText kStatusText{
    "%s: the status buffer must grow inside a stream capture; pass a status "
    "buffer or size the context first (hd_context_reserve)",
    "%s: cannot allocate status buffer"};
constexpr BufText kStageText{nullptr, "%s: cannot allocate %zu bytes of staging"};
constexpr BufText kGridText{nullptr, "%s: cannot allocate %zu bytes of user grid"};

// The context's device buffers only grow.  Growing a buffer frees the old one, which a
// captured graph may still point at, and a free/malloc cannot be captured: during
// capture growth is an error (size the context first with hd_context_reserve, or run
// the call once eagerly).  who: the entry point in the messages.
template <class T>
int ensure(hd_context* ctx, const char* who, const BufText& text, T*& p, size_t& len, size_t n) {
  if (len >= n) return HD_OK;
  if (ctx->capturing && text.capture) return fail(ctx, HD_EINVAL, text.capture, who, n * sizeof(T));
  drain(ctx);
  if (p) (void)hipFree(p);
  p = nullptr;
  len = 0;
  if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, HD_ENOMEM, text.nomem, who, n * sizeof(T));
  }
  len = n;
  return HD_OK;
}
int ensure_scratch(hd_context* ctx, const char* who, size_t ndoubles) {
  return ensure(ctx, who, kScratchText, ctx->scratch, ctx->scratch_doubles, ndoubles);
}
int ensure_pflux(hd_context* ctx, size_t ndoubles) {
  return ensure(ctx, "hd_solve_band", kPfluxText, ctx->pflux, ctx->pflux_doubles, ndoubles);
}
// the context's own per-solve status (the caller passed none)
int own_status(hd_context* ctx, const char* who, size_t nsolve, int*& status) {
  const int rc = ensure(ctx, who, kStatusText, ctx->status, ctx->status_len, nsolve);
  status = ctx->status;
  return rc;
}

// fold every recorded (K1 start, K1 end, K2 start, K2 end) quadruple into the totals
int resolve_timing(hd_context* ctx) {
  for (size_t i = 0; i + 4 <= ctx->pool_used; i += 4) {
    HD_HIP(ctx, hipEventSynchronize(ctx->pool[i + 3]));
    float t1 = 0.f, t2 = 0.f;
    HD_HIP(ctx, hipEventElapsedTime(&t1, ctx->pool[i], ctx->pool[i + 1]));
    HD_HIP(ctx, hipEventElapsedTime(&t2, ctx->pool[i + 2], ctx->pool[i + 3]));
    ctx->times.layer_ms += t1;
    ctx->times.sweep_ms += t2;
    ctx->times.layer_launches += 1;
    ctx->times.sweep_launches += 1;
  }
  ctx->pool_used = 0;
  return HD_OK;
}

// restores the caller's current device on every return path (the entry points
// switch to the context's device)
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A solve on `stream` starts after the previous solve on this context, whatever
// stream that one ran on.  Under stream capture the event is neither waited on
// nor recorded (an event recorded outside the graph cannot order a replay; a
// captured call is ordered by the stream its graph is replayed on).
int enter(hd_context* ctx, hipStream_t stream, bool* capturing) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HD_HIP(ctx, hipStreamIsCapturing(stream, &cs));
  *capturing = cs != hipStreamCaptureStatusNone;
  if (!*capturing && ctx->done_valid) HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_done, 0));
  return HD_OK;
}

int leave(hd_context* ctx, hipStream_t stream, bool capturing) {
  if (capturing) return HD_OK;
  HD_HIP(ctx, hipEventRecord(ctx->ev_done, stream));
  ctx->done_valid = true;
  return HD_OK;
}

// the stream count and the layer count of a config
enum ConfigCheck { kConfigOk, kConfigNstr, kConfigNlyr };
ConfigCheck check_config(const hd_config* cfg) {
  if (cfg->nstr < 2 || cfg->nstr % 2 || cfg->nstr / 2 > hd::kMaxNN) return kConfigNstr;
  return cfg->nlyr < 1 ? kConfigNlyr : kConfigOk;
}

// who: the name of the entry point in the messages.  out: the output array; out_optional:
// the entry point has another output it has checked itself, this one may be null
int validate(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, const double* out,
             const char* who = "hd_solve", bool out_optional = false) {
  if (!cfg || !in) return fail(ctx, HD_EINVAL, "%s: null config/inputs", who);
  switch (check_config(cfg)) {
    case kConfigNstr:
      return fail(ctx, HD_EINVAL, "%s: nstr=%d must be even and in [2, %d]", who, cfg->nstr,
                  2 * hd::kMaxNN);
    case kConfigNlyr: return fail(ctx, HD_EINVAL, "%s: nlyr=%d < 1", who, cfg->nlyr);
    case kConfigOk: break;
  }
  if (cfg->nprop < 1) return fail(ctx, HD_EINVAL, "%s: nprop=%d < 1", who, cfg->nprop);
  if (cfg->nmom < 0) return fail(ctx, HD_EINVAL, "%s: nmom=%d < 0", who, cfg->nmom);
  if (cfg->flags & ~(HD_FLAG_LAMBER | HD_FLAG_PLANCK | HD_FLAG_ONLYFL))
    return fail(ctx, HD_EINVAL, "%s: unsupported flags 0x%x", who, cfg->flags);
  if (in->nwave < 0 || in->ncol < 0)
    return fail(ctx, HD_EINVAL, "%s: negative nwave/ncol", who);
  if ((long)in->nwave * in->ncol > 0 && (!in->prop || (!out && !out_optional)))
    return fail(ctx, HD_EINVAL, "%s: prop and flux are required", who);
  if ((cfg->flags & HD_FLAG_PLANCK) && (!in->temf || !in->wave_lower || !in->wave_upper))
    return fail(ctx, HD_EINVAL, "%s: planck needs temf, wave_lower, wave_upper", who);
  if ((long)in->nwave * in->ncol > (long)0x7fffffff)
    return fail(ctx, HD_EINVAL, "%s: nwave*ncol exceeds 2^31", who);
  return HD_OK;
}

}  // namespace

namespace hd {
int set_global_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = buf;
  return code;
}
}  // namespace hd

extern "C" {

int hd_version(void) { return HDISORT_VERSION; }

// A copy per calling thread: valid until this thread's next hd_last_error call,
// whatever other threads do to the context meanwhile.
const char* hd_last_error(const hd_context* ctx_) {
  static thread_local std::string copy;
  if (ctx_) {
    hd_context* ctx = const_cast<hd_context*>(ctx_);
    std::lock_guard<std::mutex> lk(ctx->err_mu);
    copy = ctx->err;
  } else {
    std::lock_guard<std::mutex> lk(g_err_mu);
    copy = g_err;
  }
  return copy.c_str();
}

int hd_context_create(hd_context** out, int device) {
  if (!out) return fail(nullptr, HD_EINVAL, "hd_context_create: null out");
  *out = nullptr;
  DeviceGuard guard;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(nullptr, HD_EHIP, "hd_context_create: no HIP device available");
  }
  if (device < 0 || device >= ndev)
    return fail(nullptr, HD_EINVAL, "hd_context_create: device %d out of range (%d)", device,
                ndev);
  hd_context* ctx = new hd_context();
  if (const char* e = hd::ab_env("HD_JACOBI_WARM")) ctx->warm = std::atoi(e) != 0;
  if (const char* e = hd::ab_env("HD_SWEEP_QUAD")) ctx->quad = std::atoi(e) < 0 ? -1 : std::atoi(e) != 0;
  if (const char* e = hd::ab_env("HD_BAND_CMAJ")) ctx->band_cmaj = std::atoi(e) != 0;
  ctx->device = device;
  auto init = [ctx]() -> int {
    HD_HIP(ctx, hipSetDevice(ctx->device));
    HD_HIP(ctx, hipMalloc(&ctx->anyerr, sizeof(int)));
    HD_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    HD_HIP(ctx, hipStreamCreateWithFlags(&ctx->lay, hipStreamNonBlocking));
    HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming));
    HD_HIP(ctx, hipMalloc(&ctx->sink, 4096 * sizeof(double)));
    for (int b = 0; b < 2; ++b) {
      HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_layer[b], hipEventDisableTiming));
      HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_sweep[b], hipEventDisableTiming));
      HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_back[b], hipEventDisableTiming));
      HD_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_pro[b], hipEventDisableTiming));
    }
    return HD_OK;
  };
  const int rc = init();
  if (rc != HD_OK) {  // nothing leaks: destroy frees whatever init created
    std::string msg;
    {
      std::lock_guard<std::mutex> lk(ctx->err_mu);
      msg = ctx->err;
    }
    hd_context_destroy(ctx);
    return fail(nullptr, rc, "%s", msg.c_str());
  }
  *out = ctx;
  return HD_OK;
}

int hd_context_destroy(hd_context* ctx) {
  if (!ctx) return HD_OK;
  DeviceGuard guard;
  (void)hipSetDevice(ctx->device);
  drain(ctx);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->pflux) (void)hipFree(ctx->pflux);
  if (ctx->hstage) (void)hipFree(ctx->hstage);
  if (ctx->hstream) (void)hipStreamDestroy(ctx->hstream);
  if (ctx->hstream2) (void)hipStreamDestroy(ctx->hstream2);
  if (ctx->hstream3) (void)hipStreamDestroy(ctx->hstream3);
  for (int b = 0; b < 2; ++b) {
    if (ctx->hev_in[b]) (void)hipEventDestroy(ctx->hev_in[b]);
    if (ctx->hev_done[b]) (void)hipEventDestroy(ctx->hev_done[b]);
  }
  if (ctx->status) (void)hipFree(ctx->status);
  if (ctx->anyerr) (void)hipFree(ctx->anyerr);
  for (int b = 0; b < 2; ++b) {
    if (ctx->ev_layer[b]) (void)hipEventDestroy(ctx->ev_layer[b]);
    if (ctx->ev_sweep[b]) (void)hipEventDestroy(ctx->ev_sweep[b]);
    if (ctx->ev_back[b]) (void)hipEventDestroy(ctx->ev_back[b]);
    if (ctx->ev_pro[b]) (void)hipEventDestroy(ctx->ev_pro[b]);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
  if (ctx->sink) (void)hipFree(ctx->sink);
  if (ctx->rad_grid) (void)hipFree(ctx->rad_grid);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  if (ctx->lay) (void)hipStreamDestroy(ctx->lay);
  for (auto& e : ctx->pool)
    if (e) (void)hipEventDestroy(e);
  delete ctx;
  return HD_OK;
}

int hd_context_set_chunk(hd_context* ctx, long max_solves) {
  if (!ctx || max_solves < 0) return fail(ctx, HD_EINVAL, "hd_context_set_chunk: bad args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->chunk = max_solves;
  return HD_OK;
}

int hd_context_set_max_sweeps(hd_context* ctx, int max_sweeps) {
  if (!ctx || max_sweeps < 0 || max_sweeps > 64)
    return fail(ctx, HD_EINVAL, "hd_context_set_max_sweeps: bad args");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->max_sweeps = max_sweeps > 0 ? max_sweeps : 16;
  return HD_OK;
}

int hd_context_set_timing(hd_context* ctx, int enable) {
  if (!ctx) return fail(nullptr, HD_EINVAL, "hd_context_set_timing: null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->timing = enable != 0;
  ctx->pool_used = 0;  // (re)start accumulating
  ctx->times = hd_timing{};
  return HD_OK;
}

int hd_context_get_timing(const hd_context* ctx_, hd_timing* out) {
  if (!ctx_ || !out) return fail(nullptr, HD_EINVAL, "hd_context_get_timing: null arg");
  hd_context* ctx = const_cast<hd_context*>(ctx_);
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = resolve_timing(ctx);
  if (rc) return rc;
  *out = ctx->times;
  return HD_OK;
}

int hd_context_reserve(hd_context* ctx, const hd_config* cfg, long nsolve) {
  if (!ctx || !cfg || nsolve < 0) return fail(ctx, HD_EINVAL, "hd_context_reserve: bad args");
  if (check_config(cfg)) return fail(ctx, HD_EINVAL, "hd_context_reserve: bad config");
  std::lock_guard<std::mutex> lk(ctx->mu);
  DeviceGuard guard;
  HD_HIP(ctx, hipSetDevice(ctx->device));
  const int nn = cfg->nstr / 2;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const long chunk = ctx->chunk > 0 ? std::min(ctx->chunk, nsolve)
                                    : max_auto_chunk(nsolve, nn, cfg->nlyr, planck);
  int rc = ensure_scratch(ctx, "hd_solve",
                          hd::solve_reserve_doubles(nn, cfg->nlyr, planck, std::max<long>(chunk, 1)));
  if (rc) return rc;
  // and hd_solve_band's row-major route (largest call that takes it: nsolve itself)
  if (band_rowmajor(ctx, nn, nsolve)) {
    rc = ensure_pflux(ctx, (size_t)nsolve * 2 * (size_t)(cfg->nlyr + 1));
    if (rc) return rc;
  }
  rc = ensure_tables(ctx);
  if (rc) return rc;
  int* st = nullptr;
  return own_status(ctx, "hd_solve", (size_t)nsolve, st);
}

long hd_chunk_solves(const hd_config* cfg, long nsolve) {
  if (!cfg || nsolve < 0 || check_config(cfg)) return -1;
  return auto_chunk(nsolve, cfg->nstr / 2, cfg->nlyr, (cfg->flags & HD_FLAG_PLANCK) != 0);
}

int hd_quadrature(int nstr, double* mu, double* w) {
  if (nstr < 2 || nstr % 2 || !mu || !w)
    return fail(nullptr, HD_EINVAL, "hd_quadrature: bad args");
  gauss01(nstr / 2, mu, w);
  return HD_OK;
}

}  // extern "C"

namespace {

// ---- argument builders shared by the enqueue functions ------------------------------

// moments the kernels use; the delta-M rule of the prologue kernels (TaucArgs,
// FlxLevelArgs): active when chi_nstr is among them, in prop slot 1 + nstr
int used_moments(const hd_config* cfg) { return std::max(0, std::min(cfg->nmom, cfg->nprop - 2)); }

// cmaj: column-major chunk order (hd_solve_band's fused epilogue on the register path)
hd::PlanckArgs planck_args(const hd_config* cfg, const hd_inputs* in, double* out, long s0,
                           int nsc, int cmaj = 0) {
  hd::PlanckArgs pa{};
  pa.temf = in->temf;
  pa.btemp = in->btemp;
  pa.ttemp = in->ttemp;
  pa.temis = in->temis;
  pa.wlo = in->wave_lower;
  pa.whi = in->wave_upper;
  pa.out = out;
  pa.s0 = s0;
  pa.nsc = nsc;
  pa.ncol = in->ncol;
  pa.nlyr = cfg->nlyr;
  pa.cmaj = cmaj;
  pa.nwave = in->nwave;
  return pa;
}

hd::TaucArgs tauc_args(const hd_config* cfg, const hd_inputs* in, double* out, long s0, int nsc,
                       int cmaj = 0) {
  hd::TaucArgs ta{};
  ta.prop = in->prop;
  ta.out = out;
  ta.s0 = s0;
  ta.nsc = nsc;
  ta.nlyr = cfg->nlyr;
  ta.nprop = cfg->nprop;
  ta.use_f = used_moments(cfg) >= cfg->nstr;
  ta.f_slot = 1 + cfg->nstr;
  ta.cmaj = cmaj;
  ta.nwave = in->nwave;
  ta.ncol = in->ncol;
  return ta;
}

// The chunk's timing quadruple (layer start / end, sweep start / end) from the event
// pool, or null with timing off.
int timing_quad(hd_context* ctx, hipEvent_t** ev) {
  *ev = nullptr;
  if (!ctx->timing) return HD_OK;
  if (ctx->pool_used >= 4 * 512) {
    const int rc = resolve_timing(ctx);
    if (rc) return rc;
  }
  while (ctx->pool.size() < ctx->pool_used + 4) {
    hipEvent_t e;
    HD_HIP(ctx, hipEventCreate(&e));
    ctx->pool.push_back(e);
  }
  *ev = &ctx->pool[ctx->pool_used];
  ctx->pool_used += 4;
  return HD_OK;
}
// launch() on `st` between events i and i + 1 of the quadruple: i = 0 the layer kernel,
// i = 2 the sweep
template <class Launch>
hipError_t timed(hipEvent_t* ev, int i, hipStream_t st, Launch&& launch) {
  if (!ev) return launch();
  const hipError_t r0 = hipEventRecord(ev[i], st);
  const hipError_t e = launch();
  const hipError_t r1 = hipEventRecord(ev[i + 1], st);
  return e != hipSuccess ? e : (r0 != hipSuccess ? r0 : r1);
}

// ---- hd_solve, hd_solve_flx, hd_solve_band ------------------------------------------

// One call's shared setup: what the pipelines below (one function per path) launch from.
// flx (hd_solve_flx; flux and band null): the same chunks and streams with the flx
// instantiations -- register path hd_layer_kernel -> hd_sweep_flx_kernel ->
// hd_backsub_flx_kernel / _tail_kernel (never the NN-lane sweep),
// team path hd_team_mfma_layer_kernel -> hd_team_mfma_sweep_flx_kernel -- over the wider
// back-substitution records, plus the per-level prologue hd_flx_level_kernel, whose
// output only the sweep (surface level) and the back-substitution read.
struct SolveCall {
  hd_context* ctx;
  const hd_config* cfg;
  const hd_inputs* in;
  double* flux;
  double* flx;
  const hd_band* band;
  const hd_sphere* sph;  // pseudo-spherical beam (hd_solve_spher, hd_solve_flx_spher) or null
  int* status;
  hipStream_t stream;
  const char* who;  // the entry point in the messages
  long nsolve, chunk;
  int nn, nlyr;
  int nm;     // moments used
  int cmaj;   // column-major chunk order (solve_of): the fused band epilogue, register path
  int nslot;  // band: column slots per wave
  bool planck, reg;
  // Without Planck emission the layer kernels' beam sources are for a unit beam at
  // the layer top and the sweep scales them by exp(-tau_c/mu0) from its own running
  // depth, so no chunk needs the cumulative-depth prologue.  Register path: it sat
  // on the side stream behind the previous back-substitution and held each chunk's
  // layer kernel back until the sweep beside it was done.  Team path: chunk k+1's
  // prologue, launched as chunk k's sweep, waited for SIMDs the sweep's two
  // 254-register waves hold (up to 3.3 ms of a 48 ms C5 step,
  // profiles/r04/c5_timeline_last_step_v2.txt).  With Planck the sources mix beam
  // and thermal terms and the prologue stays.
  bool beam_in_sweep, need_tauc;
  bool need_pro;  // prologue output the layer kernel reads
  bool any_pro;   // ... or the sweep / back-substitution
  hd::SolvePlan plan;

  double* at(hd::SolveRegion r, int buf) const { return plan.at(ctx->scratch, r, buf); }
  int nsc_at(long s0) const { return (int)std::min(chunk, nsolve - s0); }
  long nchunk() const { return (nsolve + chunk - 1) / chunk; }

  hd::LayerArgs layer_args(long s0, int nsc, int buf) const {
    hd::LayerArgs la{};
    la.prop = in->prop;
    la.tauc = need_tauc ? at(hd::kRTauc, buf) : nullptr;  // null with a beam: unit beam at the top
    la.fbeam = in->fbeam;
    la.umu0 = in->umu0;
    la.planckv = at(hd::kRPlanck, buf);
    la.scr = at(hd::kRLayer, buf);
    la.status = status;
    la.anyerr = ctx->anyerr;
    la.s0 = s0;
    la.nsc = nsc;
    la.ncol = in->ncol;
    la.nlyr = nlyr;
    la.nprop = cfg->nprop;
    la.nmom = nm;
    la.planck = planck;
    la.max_sweeps = ctx->max_sweeps;
    la.warm = ctx->warm;
    la.sink = ctx->sink;
    la.cmaj = cmaj;
    la.nwave = in->nwave;
    return la;
  }
  hd::SweepArgs sweep_args(long s0, int nsc, int buf) const {
    hd::SweepArgs sa{};
    sa.scr = at(hd::kRLayer, buf);
    sa.bsub = at(hd::kRBsub, buf);
    sa.xsurf = at(hd::kRXsurf, buf);
    sa.flux = flux;
    sa.fbeam = in->fbeam;
    sa.umu0 = in->umu0;
    sa.albedo = in->albedo;
    sa.fisot = in->fisot;
    sa.planckv = at(hd::kRPlanck, buf);
    sa.status = status;
    sa.anyerr = ctx->anyerr;
    sa.s0 = s0;
    sa.nsc = nsc;
    sa.ncol = in->ncol;
    sa.nlyr = nlyr;
    sa.planck = planck;
    sa.sink = ctx->sink;
    sa.cmaj = cmaj;
    sa.nwave = in->nwave;
    sa.beam_scale = beam_in_sweep ? 1 : 0;
    sa.quad = ctx->quad;
    if (band && reg) {
      sa.wts = band->weight;
      sa.part = at(hd::kRPart, 0);
      sa.fsurf = at(hd::kRFsurf, buf);
      sa.nslot = nslot;
      sa.rsteps = hd::band_steps(in->nwave);
    } else if (band && !flux) {
      sa.flux = at(hd::kRFchunk, buf);
      sa.flux_local = 1;
    }
    return sa;
  }
  hd::FlxArgs flx_args(int buf) const {
    hd::FlxArgs fx{};
    fx.flx = flx;
    fx.lvl = at(hd::kRLvl, buf);
    return fx;
  }
  // the chunk's slant depths and secants (hd_spher_kernel): sub-arrays of the region,
  // interleaved with the chunk's own nsc
  hd::SphArgs sph_args(int nsc, int buf) const {
    double* q = at(hd::kRSph, buf);
    hd::SphArgs sp{};
    sp.chp = q;
    sp.lam = q + (size_t)(nlyr + 2) * nsc;
    sp.ch = flx ? q + (size_t)(2 * nlyr + 2) * nsc : nullptr;
    return sp;
  }
  hd::BandArgs band_args(long s0, int nsc, int buf) const {
    hd::BandArgs ba{};
    ba.part = at(hd::kRPart, 0);
    ba.fchunk = ba.part ? nullptr
                        : (flux ? flux + (size_t)s0 * 2 * (size_t)(nlyr + 1) : at(hd::kRFchunk, buf));
    ba.wts = band->weight;
    ba.bflux = band->bflux;
    ba.s0 = s0;
    ba.nsc = nsc;
    ba.ncol = in->ncol;
    ba.nwave = in->nwave;
    ba.nlev = nlyr + 1;
    ba.nslot = nslot;
    return ba;
  }

  // a chunk's prologue on `st`: the tauc / planck kernels the call needs and, for
  // hd_solve_flx, the chunk's per-level prologue beside them
  int prologue(long s0, int nsc, int buf, hipStream_t st) const {
    const hd::PlanckArgs pa = planck_args(cfg, in, at(hd::kRPlanck, buf), s0, nsc, cmaj);
    const hd::TaucArgs ta = tauc_args(cfg, in, at(hd::kRTauc, buf), s0, nsc, cmaj);
    HD_HIP(ctx, hd::launch_prologue(planck ? &pa : nullptr, need_tauc ? &ta : nullptr, st));
    const hd::SphArgs sp = sph ? sph_args(nsc, buf) : hd::SphArgs{};
    if (sph) {
      hd::SpherProArgs xa{};
      xa.prop = in->prop;
      xa.fbeam = in->fbeam;
      xa.umu0 = in->umu0;
      xa.zd = sph->zd;
      xa.chp = const_cast<double*>(sp.chp);
      xa.lam = const_cast<double*>(sp.lam);
      xa.ch = const_cast<double*>(sp.ch);
      xa.dts = at(hd::kRSph, buf) + (size_t)(3 * nlyr + 3) * nsc;
      xa.status = status;
      xa.anyerr = ctx->anyerr;
      xa.radius = sph->radius;
      xa.s0 = s0;
      xa.nsc = nsc;
      xa.nlyr = nlyr;
      xa.nprop = cfg->nprop;
      xa.use_f = ta.use_f;
      xa.f_slot = ta.f_slot;
      xa.cmaj = cmaj;
      xa.nwave = in->nwave;
      xa.ncol = in->ncol;
      xa.per_column = sph->per_column ? 1 : 0;
      HD_HIP(ctx, hd::launch_spher_prologue(xa, st));
    }
    if (!flx) return HD_OK;
    hd::FlxLevelArgs fa{};
    fa.prop = in->prop;
    fa.fbeam = in->fbeam;
    fa.umu0 = in->umu0;
    fa.out = at(hd::kRLvl, buf);
    fa.s0 = s0;
    fa.nsc = nsc;
    fa.nlyr = nlyr;
    fa.nprop = cfg->nprop;
    fa.use_f = ta.use_f;
    fa.f_slot = ta.f_slot;
    HD_HIP(ctx, hd::launch_flx_level(fa, sph ? &sp : nullptr, st));
    return HD_OK;
  }
  // the path's kernels (pseudo-spherical: the SPHER instantiations of the plain ones)
  hipError_t layer(const hd::LayerArgs& la, int buf, hipStream_t st) const {
    const hd::SphArgs sp = sph ? sph_args(la.nsc, buf) : hd::SphArgs{};
    return hd::launch_layer(nn, la, sph ? &sp : nullptr, st);
  }
  hipError_t sweep(const hd::SweepArgs& sa, int buf, hipStream_t st) const {
    const hd::FlxArgs fx = flx_args(buf);
    const hd::SphArgs sp = sph ? sph_args(sa.nsc, buf) : hd::SphArgs{};
    return hd::launch_sweep(nn, sa, flx ? &fx : nullptr, sph ? &sp : nullptr, st);
  }
  hipError_t backsub(const hd::SweepArgs& sa, int buf, hipStream_t st, bool tail) const {
    const hd::FlxArgs fx = flx_args(buf);
    return hd::launch_backsub(nn, sa, flx ? &fx : nullptr, st, tail);
  }
  int launch_failed(hipError_t e, const char* what = "launch") const {
    return fail(ctx, HD_EHIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
  }
  // fork: the side stream sees everything the caller's stream did before this
  // call (the inputs) -- and, under stream capture, joins the graph here
  int fork() const {
    HD_HIP(ctx, hipEventRecord(ctx->ev_fork, stream));
    HD_HIP(ctx, hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    HD_HIP(ctx, hipStreamWaitEvent(ctx->lay, ctx->ev_fork, 0));
    return HD_OK;
  }
  // join: every chunk's fluxes complete (the last work on `side` of each buffer)
  int join() const {
    for (long b = 0; b < std::min<long>(nchunk(), 2); ++b)
      HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_back[b], 0));
    return HD_OK;
  }
};

// A call of one chunk, on either path, has nothing to overlap: it runs wholly on the
// caller's stream (prologue, layer kernel, sweep and, on the register path, the tail
// back-substitution), without the fork/join of the pipelines below (C1/C3 latency).
int solve_one_chunk(const SolveCall& c) {
  const int nsc = (int)c.nsolve;
  int rc = c.prologue(0, nsc, 0, c.stream);
  if (rc) return rc;
  const hd::LayerArgs la = c.layer_args(0, nsc, 0);
  const hd::SweepArgs sa = c.sweep_args(0, nsc, 0);
  hipEvent_t* ev;
  rc = timing_quad(c.ctx, &ev);
  if (rc) return rc;
  hipError_t e = timed(ev, 0, c.stream, [&] { return c.layer(la, 0, c.stream); });
  if (e == hipSuccess) e = timed(ev, 2, c.stream, [&] { return c.sweep(sa, 0, c.stream); });
  if (e == hipSuccess && c.reg) e = c.backsub(sa, 0, c.stream, true);
  if (e == hipSuccess && c.band) e = hd::launch_band_reduce(c.band_args(0, nsc, 0), c.stream);
  return e == hipSuccess ? HD_OK : c.launch_failed(e);
}

// Register path (three streams): chunk k uses buffer k&1; its layer kernel
// (stream lay) runs beside chunk k-1's sweep (the caller's stream), its
// back-substitution (side stream) beside chunk k+1's layer kernel, and chunk
// k+1's tauc/planck prologue (side stream) beside chunk k.
int solve_reg_pipeline(const SolveCall& c) {
  hd_context* ctx = c.ctx;
  hipStream_t stream = c.stream, lay = ctx->lay, side = ctx->side;
  int rc = c.fork();
  if (rc) return rc;
  if (c.any_pro) {  // the first chunk's prologue
    rc = c.prologue(0, c.nsc_at(0), 0, side);
    if (rc) return rc;
    HD_HIP(ctx, hipEventRecord(ctx->ev_pro[0], side));
  }
  long k = 0;
  for (long s0 = 0; s0 < c.nsolve; s0 += c.chunk, ++k) {
    const int nsc = c.nsc_at(s0), buf = (int)(k & 1);
    const hd::LayerArgs la = c.layer_args(s0, nsc, buf);
    const hd::SweepArgs sa = c.sweep_args(s0, nsc, buf);
    hipEvent_t* ev;
    rc = timing_quad(ctx, &ev);
    if (rc) return rc;
    // layer kernel k on `lay`: its inputs (prologue k) are in, and sweep k-2,
    // the last reader of layer records[buf], is done
    if (c.need_pro) HD_HIP(ctx, hipStreamWaitEvent(lay, ctx->ev_pro[buf], 0));
    if (k >= 2) HD_HIP(ctx, hipStreamWaitEvent(lay, ctx->ev_sweep[buf], 0));
    hipError_t e = timed(ev, 0, lay, [&] { return c.layer(la, buf, lay); });
    HD_HIP(ctx, hipEventRecord(ctx->ev_layer[buf], lay));
    if (e != hipSuccess) return c.launch_failed(e);
    // sweep k on the caller's stream: after layer k, and after back-substitution
    // k-2, the last reader of the back-substitution records[buf]
    HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_layer[buf], 0));
    if (k >= 2) HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_back[buf], 0));
    // hd_solve_flx without a prologue the layer kernel waited for: the sweep reads it
    if (c.flx && !c.need_pro) HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_pro[buf], 0));
    e = timed(ev, 2, stream, [&] { return c.sweep(sa, buf, stream); });
    if (e != hipSuccess) return c.launch_failed(e);
    HD_HIP(ctx, hipEventRecord(ctx->ev_sweep[buf], stream));
    // next chunk's prologue into the other buffer (free: the side stream already
    // waited for the sweep of chunk k-1, the last user of that buffer)
    const long s1 = s0 + c.chunk;
    if (s1 < c.nsolve && c.any_pro) {
      rc = c.prologue(s1, c.nsc_at(s1), buf ^ 1, side);
      if (rc) return rc;
      HD_HIP(ctx, hipEventRecord(ctx->ev_pro[buf ^ 1], side));
    }
    HD_HIP(ctx, hipStreamWaitEvent(side, ctx->ev_sweep[buf], 0));
    // The last chunk's back-substitution takes the uncapped tail kernel (nothing
    // overlaps it).  With at most three chunks every chunk's does: the capped
    // kernel then still runs beside the last layer kernel when the step could
    // end, while the tail kernel takes the SIMDs briefly and is done -- 8-GPU
    // rank shape (80 000 solves, 2 chunks) 9.47 -> 10.50 M solves/s, 4-GPU
    // (160 000, 3 chunks) 10.0 -> 10.3 M; with 5 and 10 chunks the capped kernel
    // hidden under the next layer kernel stays ahead (profiles/r02_tail_ab/)
    const bool tail = s1 >= c.nsolve || c.nchunk() <= 3;
    e = c.backsub(sa, buf, side, tail);
    if (e == hipSuccess && c.band) e = hd::launch_band_reduce(c.band_args(s0, nsc, buf), side);
    if (e != hipSuccess) return c.launch_failed(e, "back-substitution launch");
    HD_HIP(ctx, hipEventRecord(ctx->ev_back[buf], side));
  }
  return c.join();
}

// Team path with several chunks: chunk k+1's prologue and layer kernel on the
// `lay` stream beside chunk k's sweep on the caller's stream.
int solve_team_pipeline(const SolveCall& c) {
  hd_context* ctx = c.ctx;
  hipStream_t stream = c.stream, lay = ctx->lay, side = ctx->side;
  int rc = c.fork();
  if (rc) return rc;
  long k = 0;
  for (long s0 = 0; s0 < c.nsolve; s0 += c.chunk, ++k) {
    const int nsc = c.nsc_at(s0), buf = (int)(k & 1);
    // buffer `buf` is free once sweep k-2 (its last reader) is done
    if (k >= 2) HD_HIP(ctx, hipStreamWaitEvent(lay, ctx->ev_sweep[buf], 0));
    rc = c.prologue(s0, nsc, buf, lay);
    if (rc) return rc;
    const hd::LayerArgs la = c.layer_args(s0, nsc, buf);
    const hd::SweepArgs sa = c.sweep_args(s0, nsc, buf);
    hipEvent_t* ev;
    rc = timing_quad(ctx, &ev);
    if (rc) return rc;
    hipError_t e = timed(ev, 0, lay, [&] { return c.layer(la, buf, lay); });
    HD_HIP(ctx, hipEventRecord(ctx->ev_layer[buf], lay));
    if (e != hipSuccess) return c.launch_failed(e);
    HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_layer[buf], 0));
    // the chunk flux buffer[buf] is free once band reduce k-2 (its reader) is done
    if (c.band && k >= 2) HD_HIP(ctx, hipStreamWaitEvent(stream, ctx->ev_back[buf], 0));
    e = timed(ev, 2, stream, [&] { return c.sweep(sa, buf, stream); });
    HD_HIP(ctx, hipEventRecord(ctx->ev_sweep[buf], stream));
    // the band reduce of chunk k on the side stream: on the caller's stream it sat
    // between sweep k and sweep k+1 waiting for SIMDs the co-running layer kernel
    // held (6.4 ms average per 11 us launch, profiles/r04/c5_kernel_stats_final.csv);
    // the reduces stay in chunk order (bflux accumulates chunk by chunk)
    if (e == hipSuccess && c.band) {
      HD_HIP(ctx, hipStreamWaitEvent(side, ctx->ev_sweep[buf], 0));
      e = hd::launch_band_reduce(c.band_args(s0, nsc, buf), side);
      HD_HIP(ctx, hipEventRecord(ctx->ev_back[buf], side));
    }
    if (e != hipSuccess) return c.launch_failed(e);
  }
  return c.band ? c.join() : HD_OK;
}

// hd_solve's enqueue body: everything it launches ends on `stream` (the side
// and lay streams fork from it and join back into it).  flux / flx / band: hd_solve,
// hd_solve_flx (flx alone) and hd_solve_band (band, flux optional).
int solve_enqueue(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flux,
                  double* flx, const hd_band* band, int*& status, hipStream_t stream,
                  const hd_sphere* sph = nullptr) {
  const long nsolve = (long)in->nwave * in->ncol;
  const int nn = cfg->nstr / 2;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const bool reg = nn <= hd::kMaxRegNN;
  const bool beam = in->fbeam != nullptr;
  const long chunk =
      ctx->chunk > 0 ? std::min(ctx->chunk, nsolve) : auto_chunk(nsolve, nn, cfg->nlyr, planck);
  // pseudo-spherical: the layer kernel always reads the prologue's secants and slant
  // depths (its records carry the attenuated sources), never the plane-parallel depths
  const bool beam_in_sweep = beam && !planck && !sph;
  const bool need_tauc = beam && !beam_in_sweep && !sph;
  const bool need_pro = planck || need_tauc || sph;
  const bool any_pro = need_pro || flx;
  SolveCall c{ctx, cfg, in, flux, flx, band, sph, status, stream,
              /*who=*/sph ? (flx ? "hd_solve_flx_spher" : "hd_solve_spher")
                          : (flx ? "hd_solve_flx" : "hd_solve"),
              nsolve, chunk, nn, cfg->nlyr,
              /*nm=*/used_moments(cfg),
              /*cmaj=*/band && reg ? 1 : 0,
              /*nslot=*/band ? hd::band_slots(in->nwave) : 0,
              planck, reg, beam_in_sweep, need_tauc, need_pro, any_pro,
              hd::SolvePlan(nn, cfg->nlyr, planck, flx != nullptr,
                            hd::band_scratch(nn, band != nullptr, flux != nullptr), in->nwave,
                            chunk, sph != nullptr)};
  int rc = ensure_scratch(ctx, c.who, c.plan.total);
  if (rc) return rc;
  rc = ensure_tables(ctx);
  if (rc) return rc;
  if (!status && (rc = own_status(ctx, c.who, (size_t)nsolve, status))) return rc;
  c.status = status;
  HD_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int) * nsolve, stream));
  HD_HIP(ctx, hipMemsetAsync(ctx->anyerr, 0, sizeof(int), stream));
  if (nsolve <= chunk) return solve_one_chunk(c);
  return reg ? solve_reg_pipeline(c) : solve_team_pipeline(c);
}

// The common frame of the two solve entry points: context lock, device guard,
// ordering behind the context's previous solve, and the synchronous error
// check when the caller passed no status buffer.
template <class Enqueue>
int run_solve(hd_context* ctx, int* status, void* stream_, const char* what, Enqueue&& enqueue) {
  DeviceGuard guard;
  HD_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  bool capturing = false;
  int rc = enter(ctx, stream, &capturing);
  if (rc) return rc;
  const bool sync = status == nullptr;
  ctx->capturing = capturing;
  rc = enqueue(status, stream);
  ctx->capturing = false;
  int any = 0;
  if (rc == HD_OK && sync) {
    const hipError_t e = hipMemcpyAsync(&any, ctx->anyerr, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (e != hipSuccess) rc = fail(ctx, HD_EHIP, "%s: anyerr copy: %s", what, hipGetErrorString(e));
  }
  const int rc2 = leave(ctx, stream, capturing);  // also after a partial enqueue
  if (rc) return rc;
  if (rc2) return rc2;
  if (sync) {
    HD_HIP(ctx, hipStreamSynchronize(stream));
    if (any)
      return fail(ctx, HD_ENUMERIC,
                  "%s: at least one solve failed (bad input, eigen breakdown or non-finite "
                  "result); DisortWrapper::Run failed.", what);
  }
  return HD_OK;
}

// The frame of every device-array solve entry point: null context, the context lock,
// the argument checks (check(): the entry point's own, then validate, in the entry
// point's order), nothing to do for an empty call, run_solve.
template <class Check, class Enqueue>
int solve_entry(hd_context* ctx, const char* who, const hd_inputs* in, int* status, void* stream,
                Check&& check, Enqueue&& enqueue) {
  if (!ctx) return fail(nullptr, HD_EINVAL, "%s: null context", who);
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = check();
  if (rc) return rc;
  if ((long)in->nwave * in->ncol == 0) return HD_OK;
  return run_solve(ctx, status, stream, who, enqueue);
}

}  // namespace

extern "C" {

int hd_solve(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flux,
             int* status, void* stream) {
  return solve_entry(
      ctx, "hd_solve", in, status, stream, [&] { return validate(ctx, cfg, in, flux); },
      [&](int*& st, hipStream_t s) {
        return solve_enqueue(ctx, cfg, in, flux, nullptr, nullptr, st, s);
      });
}

int hd_solve_flx(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flx,
                 int* status, void* stream) {
  return solve_entry(
      ctx, "hd_solve_flx", in, status, stream,
      [&] {
        const int rc = validate(ctx, cfg, in, flx, "hd_solve_flx");
        if (rc || (long)in->nwave * in->ncol == 0) return rc;
        if (reinterpret_cast<uintptr_t>(flx) % 16)
          return fail(ctx, HD_EINVAL, "hd_solve_flx: flx must be 16-byte aligned");
        return HD_OK;
      },
      [&](int*& st, hipStream_t s) {
        return solve_enqueue(ctx, cfg, in, nullptr, flx, nullptr, st, s);
      });
}

// pseudo-spherical geometry of a call: HD_EINVAL for what the host can see
static int check_sphere(hd_context* ctx, const hd_sphere* sph, const char* who) {
  if (!sph || !sph->zd) return fail(ctx, HD_EINVAL, "%s: sphere and its zd are required", who);
  if (!std::isfinite(sph->radius) || !(sph->radius > 0.0))
    return fail(ctx, HD_EINVAL, "%s: radius must be finite and > 0", who);
  return HD_OK;
}

int hd_solve_spher(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                   const hd_sphere* sph, const hd_band* band, double* flux, int* status,
                   void* stream) {
  return solve_entry(
      ctx, "hd_solve_spher", in, status, stream,
      [&] {
        if (band && (!band->weight || !band->bflux))
          return fail(ctx, HD_EINVAL, "hd_solve_spher: band weights and bflux are required");
        const int rc = check_sphere(ctx, sph, "hd_solve_spher");
        if (rc) return rc;
        return validate(ctx, cfg, in, flux, "hd_solve_spher", /*out_optional=*/band != nullptr);
      },
      [&](int*& st, hipStream_t s) {
        return solve_enqueue(ctx, cfg, in, flux, nullptr, band, st, s, sph);
      });
}

int hd_solve_flx_spher(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                       const hd_sphere* sph, double* flx, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_solve_flx_spher", in, status, stream,
      [&] {
        int rc = check_sphere(ctx, sph, "hd_solve_flx_spher");
        if (rc) return rc;
        rc = validate(ctx, cfg, in, flx, "hd_solve_flx_spher");
        if (rc || (long)in->nwave * in->ncol == 0) return rc;
        if (reinterpret_cast<uintptr_t>(flx) % 16)
          return fail(ctx, HD_EINVAL, "hd_solve_flx_spher: flx must be 16-byte aligned");
        return HD_OK;
      },
      [&](int*& st, hipStream_t s) {
        return solve_enqueue(ctx, cfg, in, nullptr, flx, nullptr, st, s, sph);
      });
}

int hd_solve_band(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                  const hd_band* band, double* flux, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_solve_band", in, status, stream,
      [&] {
        if (!band || !band->weight || !band->bflux)
          return fail(ctx, HD_EINVAL, "hd_solve_band: band weights and bflux are required");
        return validate(ctx, cfg, in, flux, "hd_solve", /*out_optional=*/true);
      },
      [&](int*& st, hipStream_t s) {
        const long nsolve = (long)in->nwave * in->ncol;
        if (flux || !band_rowmajor(ctx, cfg->nstr / 2, nsolve))
          return solve_enqueue(ctx, cfg, in, flux, nullptr, band, st, s);
        int r = ensure_pflux(ctx, (size_t)nsolve * 2 * (size_t)(cfg->nlyr + 1));
        if (r) return r;
        r = solve_enqueue(ctx, cfg, in, ctx->pflux, nullptr, nullptr, st, s);
        if (r) return r;
        r = hd_band_flux(ctx->pflux, band->weight, in->nwave, in->ncol, cfg->nlyr + 1,
                         band->bflux, s);
        return r ? fail(ctx, r, "hd_solve_band: hd_band_flux launch failed") : HD_OK;
      });
}


}  // extern "C"

namespace {

// hd_solve_host / hd_solve_band_host: the same solve on the caller's host arrays
// (pydisort's CPU-tensor contract).  The inputs go to a device staging area of
// the context, the solve runs on the context's own stream, the outputs come back;
// synchronous.  No CPU arithmetic: without a device the call fails like hd_solve.
int solve_host(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flux,
               const double* weight, double* bflux, int* status, const char* what) {
  if (!ctx) return fail(nullptr, HD_EINVAL, "%s: null context", what);
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!cfg || !in) return fail(ctx, HD_EINVAL, "%s: null config or inputs", what);
  const bool band = bflux != nullptr;
  if (band && !weight) return fail(ctx, HD_EINVAL, "%s: band weights are required", what);
  int rc = validate(ctx, cfg, in, flux, "hd_solve", /*out_optional=*/true);  // flux or bflux is given
  if (rc) return rc;
  const long nsolve = (long)in->nwave * in->ncol;
  if (nsolve == 0) return HD_OK;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const int nlev = cfg->nlyr + 1;
  const size_t nlev2 = 2 * (size_t)nlev;
  const size_t ns = (size_t)nsolve;
  const size_t ncol = (size_t)in->ncol;
  // Pieces of whole waves (contiguous slices of every input): piece j+1's arrays
  // go over PCIe (copy stream) while piece j is solved (compute stream); two input
  // buffers.  ~128 k solves per piece keeps each solve near full-batch efficiency.
  const long wpp = std::max<long>(1, std::min<long>(in->nwave, (131072 + in->ncol - 1) / in->ncol));
  const int npiece = (int)((in->nwave + wpp - 1) / wpp);
  const size_t pin_prop = (size_t)wpp * ncol * cfg->nlyr * (size_t)cfg->nprop;
  const size_t pin_bc = (size_t)wpp * ncol;
  const double* bc_h[7] = {in->fbeam, in->umu0, in->albedo, in->btemp,
                           in->ttemp, in->temis, in->fisot};
  int nbc = 0;
  for (int k = 0; k < 7; ++k) nbc += bc_h[k] != nullptr;
  const size_t pin = pin_prop + nbc * pin_bc;
  const size_t n_temf = planck ? ncol * nlev : 0;
  const size_t n_wave = planck ? (size_t)in->nwave : 0;
  const size_t n_w = band ? (size_t)in->nwave + npiece : 0;  // weights, then ones
  const size_t n_flux = flux ? ns * nlev2 : 0;
  const size_t n_part = band ? (size_t)npiece * ncol * nlev2 + ncol * nlev2 : 0;
  const size_t n_stat = (ns + 1) / 2;  // int32 in double slots
  const size_t total = 2 * pin + n_temf + 2 * n_wave + n_w + n_flux + n_part + n_stat;
  DeviceGuard guard;
  HD_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->hstream) HD_HIP(ctx, hipStreamCreateWithFlags(&ctx->hstream, hipStreamNonBlocking));
  if (!ctx->hstream2) HD_HIP(ctx, hipStreamCreateWithFlags(&ctx->hstream2, hipStreamNonBlocking));
  if (!ctx->hstream3) HD_HIP(ctx, hipStreamCreateWithFlags(&ctx->hstream3, hipStreamNonBlocking));
  for (int b = 0; b < 2; ++b) {
    if (!ctx->hev_in[b]) HD_HIP(ctx, hipEventCreateWithFlags(&ctx->hev_in[b], hipEventDisableTiming));
    if (!ctx->hev_done[b])
      HD_HIP(ctx, hipEventCreateWithFlags(&ctx->hev_done[b], hipEventDisableTiming));
  }
  rc = ensure(ctx, what, kStageText, ctx->hstage, ctx->hstage_len, total);
  if (rc) return rc;
  // uploads, solves, downloads: the per-point fluxes of piece j go back on their own
  // stream while piece j+2's arrays go up (both PCIe directions at once)
  hipStream_t cs = ctx->hstream, xs = ctx->hstream2, ds = ctx->hstream3;
  // whatever happens below, nothing may still be reading or writing the
  // caller's arrays when this returns
  struct Drain {
    hipStream_t a, b, c;
    ~Drain() {
      (void)hipStreamSynchronize(a);
      (void)hipStreamSynchronize(b);
      (void)hipStreamSynchronize(c);
    }
  } drain_on_exit{cs, xs, ds};
  double* q = ctx->hstage;
  double* inbuf[2] = {q, q + pin};
  q += 2 * pin;
  double* temf_d = n_temf ? q : nullptr;
  q += n_temf;
  double* wlo_d = n_wave ? q : nullptr;
  q += n_wave;
  double* whi_d = n_wave ? q : nullptr;
  q += n_wave;
  double* w_d = band ? q : nullptr;
  q += n_w;
  double* flux_d = flux ? q : nullptr;
  q += n_flux;
  double* part_d = band ? q : nullptr;  // [piece][ncol][nlev][2], then the band sum
  q += n_part;
  int* st_d = reinterpret_cast<int*>(q);
  auto h2d = [&](double* d, const double* h, size_t n) {
    return hipMemcpyAsync(d, h, n * sizeof(double), hipMemcpyHostToDevice, cs);
  };
  if (n_temf) HD_HIP(ctx, h2d(temf_d, in->temf, n_temf));
  if (n_wave) {
    HD_HIP(ctx, h2d(wlo_d, in->wave_lower, n_wave));
    HD_HIP(ctx, h2d(whi_d, in->wave_upper, n_wave));
  }
  if (band) {
    HD_HIP(ctx, h2d(w_d, weight, (size_t)in->nwave));
    std::vector<double> ones((size_t)npiece, 1.0);
    HD_HIP(ctx, hipMemcpy(w_d + in->nwave, ones.data(), npiece * sizeof(double),
                          hipMemcpyHostToDevice));
  }
  std::vector<int> st_h(status ? 0 : ns);
  int* st_out = status ? status : st_h.data();
  auto d2h = [&](int j) -> int {  // piece j's per-point fluxes and status, after its solve
    const long w0 = (long)j * wpp, wj = std::min<long>(wpp, in->nwave - w0);
    const size_t o = (size_t)w0 * ncol, n = (size_t)wj * ncol;
    HD_HIP(ctx, hipStreamWaitEvent(ds, ctx->hev_done[j & 1], 0));
    if (flux)
      HD_HIP(ctx, hipMemcpyAsync(flux + o * nlev2, flux_d + o * nlev2, n * nlev2 * sizeof(double),
                                 hipMemcpyDeviceToHost, ds));
    HD_HIP(ctx, hipMemcpyAsync(st_out + o, st_d + o, n * sizeof(int), hipMemcpyDeviceToHost, ds));
    return HD_OK;
  };
  for (int j = 0; j < npiece; ++j) {
    const int b = j & 1;
    const long w0 = (long)j * wpp, wj = std::min<long>(wpp, in->nwave - w0);
    const size_t o = (size_t)w0 * ncol, n = (size_t)wj * ncol;
    // buffer b was last read by the solve of piece j-2
    if (j >= 2) HD_HIP(ctx, hipStreamWaitEvent(cs, ctx->hev_done[b], 0));
    hd_inputs din = *in;
    din.nwave = (int)wj;
    double* p = inbuf[b];
    const size_t nprop = n * cfg->nlyr * (size_t)cfg->nprop;
    HD_HIP(ctx, h2d(p, in->prop + o * cfg->nlyr * (size_t)cfg->nprop, nprop));
    din.prop = p;
    p += nprop;
    const double** bc_d[7] = {&din.fbeam, &din.umu0, &din.albedo, &din.btemp,
                              &din.ttemp, &din.temis, &din.fisot};
    for (int k = 0; k < 7; ++k) {
      if (!bc_h[k]) continue;
      HD_HIP(ctx, h2d(p, bc_h[k] + o, n));
      *bc_d[k] = p;
      p += n;
    }
    din.temf = temf_d;
    din.wave_lower = wlo_d ? wlo_d + w0 : nullptr;
    din.wave_upper = whi_d ? whi_d + w0 : nullptr;
    HD_HIP(ctx, hipEventRecord(ctx->hev_in[b], cs));
    HD_HIP(ctx, hipStreamWaitEvent(xs, ctx->hev_in[b], 0));
    double* fd = flux ? flux_d + o * nlev2 : nullptr;
    rc = run_solve(ctx, st_d + o, xs, what, [&](int*& st, hipStream_t ss) {
      if (!band) return solve_enqueue(ctx, cfg, &din, fd, nullptr, nullptr, st, ss);
      hd_band bb{w_d + w0, part_d + (size_t)j * ncol * nlev2};
      return solve_enqueue(ctx, cfg, &din, fd, nullptr, &bb, st, ss);
    });
    if (rc) return rc;
    HD_HIP(ctx, hipEventRecord(ctx->hev_done[b], xs));
    if (j >= 1 && (rc = d2h(j - 1))) return rc;
  }
  if ((rc = d2h(npiece - 1))) return rc;
  if (band) {
    // the pieces' band partials, in piece (= wave) order
    double* bsum = part_d + (size_t)npiece * ncol * nlev2;
    rc = hd_band_flux(part_d, w_d + in->nwave, npiece, (int)ncol, nlev, bsum, xs);
    if (rc) return fail(ctx, rc, "%s: band sum: %s", what, hd_last_error(nullptr));
    HD_HIP(ctx, hipEventRecord(ctx->hev_done[0], xs));
    HD_HIP(ctx, hipStreamWaitEvent(ds, ctx->hev_done[0], 0));
    HD_HIP(ctx, hipMemcpyAsync(bflux, bsum, ncol * nlev2 * sizeof(double), hipMemcpyDeviceToHost, ds));
  }
  HD_HIP(ctx, hipStreamSynchronize(cs));
  HD_HIP(ctx, hipStreamSynchronize(xs));
  HD_HIP(ctx, hipStreamSynchronize(ds));
  for (size_t i = 0; i < ns; ++i)
    if (st_out[i] & HD_STATUS_ERROR_MASK)
      return fail(ctx, HD_ENUMERIC,
                  "%s: at least one solve failed (bad input, eigen breakdown or non-finite "
                  "result); DisortWrapper::Run failed.", what);
  return HD_OK;
}

}  // namespace

extern "C" {

int hd_solve_host(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flux,
                  int* status) {
  if (!flux) return fail(ctx, HD_EINVAL, "hd_solve_host: null flux");
  return solve_host(ctx, cfg, in, flux, nullptr, nullptr, status, "hd_solve_host");
}

int hd_solve_band_host(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                       const double* weight, double* bflux, double* flux, int* status) {
  if (!bflux) return fail(ctx, HD_EINVAL, "hd_solve_band_host: null bflux");
  return solve_host(ctx, cfg, in, flux, weight, bflux, status, "hd_solve_band_host");
}

}  // extern "C"

namespace {

int validate_rad(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                 const hd_radiance* rad, double* flux, double* uu, bool rays = false) {
  const char* who = rays ? "hd_solve_rays" : "hd_solve_radiance";
  int rc = validate(ctx, cfg, in, flux, who, /*out_optional=*/rays);  // rays: rad or brad is given
  if (rc) return rc;
  if (!rad) return fail(ctx, HD_EINVAL, "%s: null radiance config", who);
  const int nn = cfg->nstr / 2;
  if (nn > hd::kRadMaxNN)
    return fail(ctx, HD_EINVAL, "%s: nstr=%d; the intensity path supports nstr <= %d", who,
                cfg->nstr, 2 * hd::kRadMaxNN);
  const bool radiances = rad->onlyfl == 0;
  const int nlyr = cfg->nlyr;
  const int ntau = rad->ntau > 0 ? rad->ntau : nlyr + 1;
  const int numu = radiances ? rad->numu : 0;
  const int nphi = radiances ? rad->nphi : 0;
  if (rad->corint != 0 && rad->corint != 1)
    return fail(ctx, HD_EINVAL,
                "%s: corint=%d; 0 (none) and 1 (Nakajima-Tanaka, cdisort's "
                "old_intensity_correction) are implemented, cdisort's new correction is not",
                who, rad->corint);
  if (rad->ntau < 0 || (rad->ntau > 0 && !rad->utau))
    return fail(ctx, HD_EINVAL, "%s: ntau=%d needs utau", who, rad->ntau);
  for (int i = 0; i < rad->ntau; ++i)
    if (!(rad->utau[i] >= 0.0) || (i > 0 && !(rad->utau[i] >= rad->utau[i - 1])))
      return fail(ctx, HD_EINVAL, "%s: utau must be >= 0 and ascending", who);
  if (radiances && !rays) {
    if (numu < 1 || !rad->umu || nphi < 1 || !rad->phi || !uu)
      return fail(ctx, HD_EINVAL,
                  "hd_solve_radiance: radiances need numu >= 1, nphi >= 1, umu, phi and uu");
    for (int i = 0; i < numu; ++i)
      if (!(rad->umu[i] != 0.0) || !(std::fabs(rad->umu[i]) <= 1.0))
        return fail(ctx, HD_EINVAL, "hd_solve_radiance: umu[%d]=%g must be in [-1,0)U(0,1]", i,
                    rad->umu[i]);
  }
  return HD_OK;
}

// rays = null: the grid call (rad->umu x rad->phi, host arrays, into uu).  rays given
// (hd_solve_rays): rad is its view of them (numu = nray, nphi = 1, umu / phi unused),
// uu is the per-wave ray output or null.  sph (hd_solve_rays_spher, nstr <= 16): the
// pseudo-spherical beam -- hd_spher_kernel after the chunk's tauc / Planck prologue, with
// ch requested, and hd_rad_spher.hip's kernels.  keep_status: a solve of the same call
// already ran on `stream` and its status bits stay (hd_solve_rays_spher's level fluxes)
int rad_enqueue(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                const hd_radiance* rad, const hd_rays* rays, double* flux, double* uu,
                int*& status, hipStream_t stream, const hd_sphere* sph = nullptr,
                bool keep_status = false) {
  const char* who = rays ? (sph ? "hd_solve_rays_spher" : "hd_solve_rays") : "hd_solve_radiance";
  int rc = HD_OK;
  const int nn = cfg->nstr / 2;
  const bool radiances = rad->onlyfl == 0;
  const int nlyr = cfg->nlyr;
  const int ntau = rad->ntau > 0 ? rad->ntau : nlyr + 1;
  const int numu = radiances ? rad->numu : 0;
  const int nphi = radiances ? rad->nphi : 0;
  const long nsolve = (long)in->nwave * in->ncol;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const bool beam = in->fbeam != nullptr;
  const int nm_mode = (radiances && beam) ? cfg->nstr : 1;
  const int nmom = used_moments(cfg);

  // the user grid is copied from host arrays and its buffer may grow: a radiance
  // solve is not capturable (a replay would reread host memory the caller may have
  // freed, and nothing may be allocated under capture)
  if (ctx->capturing)
    return fail(ctx, HD_EINVAL,
                "%s: not capturable into a HIP graph (host user grid)", who);
  rc = ensure_rad_tables(ctx);
  if (rc) return rc;
  // user grid on the device: umu | phi | utau; rays: their cosines with the bad ones
  // replaced (launch_ray_cosines) | utau, the azimuths read from the caller's array
  const size_t ncos = rays ? (size_t)(rays->per_column ? in->ncol : 1) * numu : (size_t)numu;
  const size_t ngrid = rays ? ncos + rad->ntau : (size_t)numu + nphi + rad->ntau;
  rc = ensure(ctx, who, kGridText, ctx->rad_grid, ctx->rad_grid_len, ngrid);
  if (rc) return rc;
  double* d_umu = ctx->rad_grid;
  double* d_phi = d_umu + numu;
  double* d_utau = rays ? d_umu + ncos : d_phi + nphi;
  if (rays) {
    HD_HIP(ctx, hd::launch_ray_cosines(rays->umu, d_umu, (long)ncos, stream));
  } else {
    if (numu) HD_HIP(ctx, hipMemcpyAsync(d_umu, rad->umu, numu * sizeof(double), hipMemcpyHostToDevice, stream));
    if (nphi) HD_HIP(ctx, hipMemcpyAsync(d_phi, rad->phi, nphi * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  if (rad->ntau)
    HD_HIP(ctx, hipMemcpyAsync(d_utau, rad->utau, rad->ntau * sizeof(double), hipMemcpyHostToDevice, stream));

  // the intensity kernels keep the register-path layer record layout at every
  // nstr (hd::layer_record_doubles gives the team layout above nstr 16)
  const hd::RadPlan plan(nn, nlyr, planck, nm_mode, ntau, numu, hd::rad_layer_record_doubles(nn),
                         hd::rad_rec_doubles(nn), hd::rad_bsub_doubles(nn), nsolve, ctx->chunk,
                         /*spher=*/sph != nullptr);
  rc = ensure_scratch(ctx, who, plan.total);
  if (rc) return rc;
  if (!status && (rc = own_status(ctx, who, (size_t)nsolve, status))) return rc;
  if (!keep_status) {
    HD_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int) * nsolve, stream));
    HD_HIP(ctx, hipMemsetAsync(ctx->anyerr, 0, sizeof(int), stream));
  }

  double* const q = ctx->scratch;
  double *r_sw = q + plan.sw, *r_rd = q + plan.rd, *r_bs = q + plan.bs, *r_lev = q + plan.lev,
         *r_cst = q + plan.cst, *r_radm = q + plan.radm, *r_taus = q + plan.taus,
         *r_tauc = q + plan.tauc, *r_planck = planck ? q + plan.planck : nullptr;

  for (long s0 = 0; s0 < nsolve; s0 += plan.chunk) {
    const int ns = (int)std::min(plan.chunk, nsolve - s0);
    const hd::TaucArgs ta = tauc_args(cfg, in, r_tauc, s0, ns);
    const hd::PlanckArgs pa = planck_args(cfg, in, r_planck, s0, ns);
    HD_HIP(ctx, hd::launch_prologue(planck ? &pa : nullptr, beam ? &ta : nullptr, stream));
    hd::RadArgs a{};
    if (sph) {  // ch' [nlyr+2] | lambda [nlyr] | ch [nlyr+1] | staging [2][nlyr], stride ns
      double* r_sph = q + plan.sph;
      hd::SpherProArgs xa{};
      xa.prop = in->prop;
      xa.fbeam = in->fbeam;
      xa.umu0 = in->umu0;
      xa.zd = sph->zd;
      xa.chp = r_sph;
      xa.lam = r_sph + (size_t)(nlyr + 2) * ns;
      xa.ch = r_sph + (size_t)(2 * nlyr + 2) * ns;
      xa.dts = r_sph + (size_t)(3 * nlyr + 3) * ns;
      xa.status = status;
      xa.anyerr = ctx->anyerr;
      xa.radius = sph->radius;
      xa.s0 = s0;
      xa.nsc = ns;
      xa.nlyr = nlyr;
      xa.nprop = cfg->nprop;
      xa.use_f = ta.use_f;
      xa.f_slot = ta.f_slot;
      xa.cmaj = 0;
      xa.nwave = in->nwave;
      xa.ncol = in->ncol;
      xa.per_column = sph->per_column ? 1 : 0;
      HD_HIP(ctx, hd::launch_spher_prologue(xa, stream));
      a.chp = xa.chp;
      a.lam = xa.lam;
      a.ch = xa.ch;
    }
    a.prop = in->prop;
    a.fbeam = in->fbeam;
    a.umu0 = in->umu0;
    a.albedo = in->albedo;
    a.fisot = in->fisot;
    a.phi0 = rad->phi0;
    a.planckv = r_planck;
    a.tauc = beam ? r_tauc : nullptr;
    a.taus = r_taus;
    a.umu = d_umu;
    a.phi = rays ? rays->phi : d_phi;
    a.utau = rad->ntau > 0 ? d_utau : nullptr;
    a.rsw = r_sw;
    a.rrd = r_rd;
    a.bsub = r_bs;
    a.lev = r_lev;
    a.cst = r_cst;
    a.radm = r_radm;
    a.flux = flux;
    a.uu = rays ? nullptr : uu;
    if (rays) {
      a.umu_stride = rays->per_column ? numu : 0;
      a.ray_umu = rays->umu;
      a.weight = rays->weight;
      a.rad = uu;
      a.brad = rays->brad;
    }
    a.status = status;
    a.anyerr = ctx->anyerr;
    a.s0 = s0;
    a.ns = ns;
    a.nm = nm_mode;
    a.nu = ns * nm_mode;
    a.ncol = in->ncol;
    a.nlyr = nlyr;
    a.nprop = cfg->nprop;
    a.nmom = nmom;
    a.planck = planck;
    a.max_sweeps = ctx->max_sweeps;
    a.numu = numu;
    a.nphi = nphi;
    a.ntau = ntau;
    a.corint = rad->corint != 0;
    a.sink = ctx->sink;
    hipError_t e = hd::launch_rad_chunk(nn, a, radiances, stream);
    if (e != hipSuccess)
      return fail(ctx, HD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  }
  return HD_OK;
}

}  // namespace

extern "C" {

int hd_solve_radiance(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                      const hd_radiance* rad, double* flux, double* uu, int* status,
                      void* stream) {
  return solve_entry(
      ctx, "hd_solve_radiance", in, status, stream,
      [&] { return validate_rad(ctx, cfg, in, rad, flux, uu); },
      [&](int*& st, hipStream_t s) {
        return rad_enqueue(ctx, cfg, in, rad, nullptr, flux, uu, st, s);
      });
}

int hd_solve_rays(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                  const hd_rays* rays, double* flux, double* rad, int* status, void* stream) {
  hd_radiance view{};  // the rays as hd_solve_radiance's user grid
  return solve_entry(
      ctx, "hd_solve_rays", in, status, stream,
      [&] {
        if (!rays) return fail(ctx, HD_EINVAL, "hd_solve_rays: null ray config");
        if (!rad && !rays->brad)
          return fail(ctx, HD_EINVAL, "hd_solve_rays: rad and brad both NULL: nothing to compute");
        if (rays->brad && !rays->weight)
          return fail(ctx, HD_EINVAL, "hd_solve_rays: brad needs weight");
        if (rays->nray < 1 || !rays->umu || !rays->phi)
          return fail(ctx, HD_EINVAL, "hd_solve_rays: rays need nray >= 1, umu and phi");
        if (rays->per_column != 0 && rays->per_column != 1)
          return fail(ctx, HD_EINVAL, "hd_solve_rays: per_column=%d must be 0 or 1",
                      rays->per_column);
        // the rest as hd_solve_radiance (nstr, ntau/utau, corint); the cosines are device
        // data, checked by the kernels
        view.ntau = rays->ntau;
        view.utau = rays->utau;
        view.numu = rays->nray;
        view.nphi = 1;
        view.phi0 = rays->phi0;
        view.onlyfl = 0;
        view.corint = rays->corint;
        return validate_rad(ctx, cfg, in, &view, flux, rad ? rad : rays->brad, /*rays=*/true);
      },
      [&](int*& st, hipStream_t s) {
        return rad_enqueue(ctx, cfg, in, &view, rays, flux, rad, st, s);
      });
}

int hd_solve_rays_spher(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                        const hd_sphere* sph, const hd_rays* rays, double* flux, double* rad,
                        int* status, void* stream) {
  hd_radiance view{};  // the rays as hd_solve_radiance's user grid
  return solve_entry(
      ctx, "hd_solve_rays_spher", in, status, stream,
      [&] {
        const char* who = "hd_solve_rays_spher";
        if (!rays) return fail(ctx, HD_EINVAL, "%s: null ray config", who);
        if (!rad && !rays->brad)
          return fail(ctx, HD_EINVAL, "%s: rad and brad both NULL: nothing to compute", who);
        if (rays->brad && !rays->weight) return fail(ctx, HD_EINVAL, "%s: brad needs weight", who);
        if (rays->nray < 1 || !rays->umu || !rays->phi)
          return fail(ctx, HD_EINVAL, "%s: rays need nray >= 1, umu and phi", who);
        if (rays->per_column != 0 && rays->per_column != 1)
          return fail(ctx, HD_EINVAL, "%s: per_column=%d must be 0 or 1", who, rays->per_column);
        int rc = check_sphere(ctx, sph, who);
        if (rc) return rc;
        if (cfg && cfg->nstr > 2 * hd::kMaxRegNN)
          return fail(ctx, HD_EINVAL,
                      "%s: nstr=%d; pseudo-spherical ray radiances support nstr <= %d", who,
                      cfg->nstr, 2 * hd::kMaxRegNN);
        view.ntau = rays->ntau;
        view.utau = rays->utau;
        view.numu = rays->nray;
        view.nphi = 1;
        view.phi0 = rays->phi0;
        view.onlyfl = 0;
        view.corint = rays->corint;
        return validate_rad(ctx, cfg, in, &view, flux, rad ? rad : rays->brad, /*rays=*/true);
      },
      [&](int*& st, hipStream_t s) {
        // Fluxes at the layer boundaries are hd_solve_spher's own: the flux solve runs
        // first on the same stream and scratch, so one model's two outputs -- the fluxes
        // of a flux module and those along the rays -- are the same numbers, bit for bit.
        // Fluxes at user depths (utau) come from the intensity path's flux kernel.
        const bool level_flux = flux && rays->ntau == 0;
        if (level_flux) {
          if (ctx->capturing)
            return fail(ctx, HD_EINVAL,
                        "hd_solve_rays_spher: not capturable into a HIP graph (host user grid)");
          const int rc = solve_enqueue(ctx, cfg, in, flux, nullptr, nullptr, st, s, sph);
          if (rc) return rc;
        }
        return rad_enqueue(ctx, cfg, in, &view, rays, level_flux ? nullptr : flux, rad, st, s, sph,
                           /*keep_status=*/level_flux);
      });
}

}  // extern "C"

// ============================================================================
// Beer-Lambert solver (include/hdbeer.h; kernels in hd_beer.hip)
// ============================================================================
namespace {

// flux given / band given: hd_beer_flux(_band); rays given: hd_beer_rays (out = rad)
int beer_enqueue(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* out,
                 const hd_band* band, const struct hd_beer_rays* rays, int*& status,
                 hipStream_t stream, const char* who) {
  int rc = HD_OK;
  const long nsolve = (long)in->nwave * in->ncol;
  const int nn = cfg->nstr / 2;
  const int nlyr = cfg->nlyr;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const size_t m = rays ? (size_t)rays->nray : 2 * (size_t)(nlyr + 1);  // values per solve
  const double* weight = rays ? rays->weight : (band ? band->weight : nullptr);
  double* bout = rays ? rays->brad : (band ? band->bflux : nullptr);
  const hd::BeerPlan plan(nlyr, planck, rays != nullptr, out != nullptr, m, nsolve, ctx->chunk);
  rc = ensure_scratch(ctx, who, plan.total);
  if (rc) return rc;
  if (!status && (rc = own_status(ctx, who, (size_t)nsolve, status))) return rc;
  HD_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int) * nsolve, stream));
  HD_HIP(ctx, hipMemsetAsync(ctx->anyerr, 0, sizeof(int), stream));
  if (bout) HD_HIP(ctx, hipMemsetAsync(bout, 0, sizeof(double) * in->ncol * m, stream));
  double* planck_q = planck ? ctx->scratch + plan.planck : nullptr;
  double* xsurf_q = ctx->scratch + plan.xsurf;
  double* local_q = ctx->scratch + plan.local;
  const hd::QuadHost& q = quad_host()[nn - 1];
  for (long s0 = 0; s0 < nsolve; s0 += plan.chunk) {
    const int nsc = (int)std::min(plan.chunk, nsolve - s0);
    if (planck) {
      const hd::PlanckArgs pa = planck_args(cfg, in, planck_q, s0, nsc);
      HD_HIP(ctx, hd::launch_prologue(&pa, nullptr, stream));
    }
    double* vals = out ? out + (size_t)s0 * m : local_q;  // the chunk's per-wave values
    hd::BeerArgs a{};
    a.prop = in->prop;
    a.fbeam = in->fbeam;
    a.umu0 = in->umu0;
    a.albedo = in->albedo;
    a.fisot = in->fisot;
    a.planckv = planck_q;
    a.flux = rays ? nullptr : vals;
    a.xsurf = rays ? xsurf_q : nullptr;
    a.status = status;
    a.anyerr = ctx->anyerr;
    a.s0 = s0;
    a.nsc = nsc;
    a.nlyr = nlyr;
    a.nprop = cfg->nprop;
    for (int i = 0; i < nn; ++i) {
      a.rmu[i] = 1.0 / q.mu[i];
      a.wmu[i] = q.w[i] * q.mu[i];
    }
    hipError_t e;
    if (!rays) {
      e = hd::launch_beer_flux(nn, a, stream);
    } else {
      e = hd::launch_beer_surface(nn, a, stream);
      if (e == hipSuccess) {
        hd::BeerRayArgs r{};
        r.prop = in->prop;
        r.albedo = in->albedo;
        r.fisot = in->fisot;
        r.planckv = planck_q;
        r.xsurf = xsurf_q;
        r.umu = rays->umu;
        r.rad = vals;
        r.status = status;
        r.anyerr = ctx->anyerr;
        r.s0 = s0;
        r.nsc = nsc;
        r.ncol = in->ncol;
        r.nlyr = nlyr;
        r.nprop = cfg->nprop;
        r.nray = rays->nray;
        r.per_column = rays->per_column;
        r.alpha = rays->alpha;
        e = hd::launch_beer_rays(r, stream);
      }
    }
    if (e == hipSuccess && bout)
      e = hd::launch_beer_band_acc(vals, weight, bout, s0, nsc, in->ncol, (long)m, stream);
    if (e != hipSuccess)
      return fail(ctx, HD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  }
  return HD_OK;
}

// the argument checks the two gradient entry points share
int beer_bwd_check(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                   const hd_beer_cot* cot, const hd_beer_grads* g, const char* who) {
  const int rc = validate(ctx, cfg, in, nullptr, who, /*out_optional=*/true);
  if (rc) return rc;
  if (!cot || !g) return fail(ctx, HD_EINVAL, "%s: null cotangent or gradient set", who);
  if (cot->per_wave ? (cot->band || cot->weight) : (!cot->band || !cot->weight))
    return fail(ctx, HD_EINVAL, "%s: the cotangent is either per_wave or band with weight", who);
  if (!(cfg->flags & HD_FLAG_PLANCK) && (g->gtemf || g->g_btemp || g->g_ttemp))
    return fail(ctx, HD_EINVAL, "%s: gtemf, g_btemp and g_ttemp need HD_FLAG_PLANCK", who);
  if ((g->g_albedo && !in->albedo) || (g->g_fbeam && !in->fbeam) || (g->g_umu0 && !in->umu0) ||
      (g->g_btemp && !in->btemp) || (g->g_ttemp && !in->ttemp) || (g->g_temis && !in->temis) ||
      (g->g_fisot && !in->fisot))
    return fail(ctx, HD_EINVAL, "%s: a boundary gradient needs that boundary input", who);
  return HD_OK;
}

// rays null: hd_beer_flux_bwd; given: hd_beer_rays_bwd
int beer_bwd_enqueue(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                     const struct hd_beer_rays* rays, const hd_beer_cot* cot,
                     const hd_beer_grads* g, int*& status, hipStream_t stream, const char* who) {
  int rc = HD_OK;
  const long nsolve = (long)in->nwave * in->ncol;
  const int nn = cfg->nstr / 2;
  const int nlyr = cfg->nlyr;
  const bool planck = (cfg->flags & HD_FLAG_PLANCK) != 0;
  const hd::BeerGradPlan plan(nn, nlyr, planck, rays != nullptr, nsolve, ctx->chunk);
  rc = ensure_scratch(ctx, who, plan.total);
  if (rc) return rc;
  if (!status && (rc = own_status(ctx, who, (size_t)nsolve, status))) return rc;
  HD_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int) * nsolve, stream));
  HD_HIP(ctx, hipMemsetAsync(ctx->anyerr, 0, sizeof(int), stream));
  if (g->gtemf)
    HD_HIP(ctx, hipMemsetAsync(g->gtemf, 0, sizeof(double) * in->ncol * (nlyr + 1), stream));
  if (g->g_temis && !planck)
    HD_HIP(ctx, hipMemsetAsync(g->g_temis, 0, sizeof(double) * nsolve, stream));
  double* planck_q = planck ? ctx->scratch + plan.planck : nullptr;
  double* gb_q = planck ? ctx->scratch + plan.gb : nullptr;
  double* seed_q = ctx->scratch + plan.seed;
  const hd::QuadHost& q = quad_host()[nn - 1];
  const hd::BeerCot kcot{cot->per_wave, cot->band, cot->weight};
  for (long s0 = 0; s0 < nsolve; s0 += plan.chunk) {
    const int nsc = (int)std::min(plan.chunk, nsolve - s0);
    if (planck) {
      const hd::PlanckArgs pa = planck_args(cfg, in, planck_q, s0, nsc);
      HD_HIP(ctx, hd::launch_prologue(&pa, nullptr, stream));
    }
    hd::BeerBwdArgs a{};
    a.prop = in->prop;
    a.fbeam = in->fbeam;
    a.umu0 = in->umu0;
    a.albedo = in->albedo;
    a.fisot = in->fisot;
    a.planckv = planck_q;
    a.sweep = ctx->scratch + plan.sweep;
    a.gb = gb_q;
    a.gtau = g->gtau;
    a.g_albedo = g->g_albedo;
    a.g_fbeam = g->g_fbeam;
    a.g_umu0 = g->g_umu0;
    a.g_fisot = g->g_fisot;
    a.status = status;
    a.anyerr = ctx->anyerr;
    a.s0 = s0;
    a.nsc = nsc;
    a.ncol = in->ncol;
    a.nlyr = nlyr;
    a.nprop = cfg->nprop;
    for (int i = 0; i < nn; ++i) {
      a.rmu[i] = 1.0 / q.mu[i];
      a.wmu[i] = q.w[i] * q.mu[i];
    }
    hipError_t e;
    if (!rays) {
      a.cot = kcot;
      e = hd::launch_beer_flux_bwd(nn, a, stream);
    } else {
      // the forward's surface intensity into the seed region, then the rays' adjoint
      // (which replaces it by the seed), then the adjoint of the down pass
      hd::BeerArgs f{};
      f.prop = in->prop;
      f.fbeam = in->fbeam;
      f.umu0 = in->umu0;
      f.albedo = in->albedo;
      f.fisot = in->fisot;
      f.planckv = planck_q;
      f.xsurf = seed_q;
      f.status = status;
      f.anyerr = ctx->anyerr;
      f.s0 = s0;
      f.nsc = nsc;
      f.nlyr = nlyr;
      f.nprop = cfg->nprop;
      for (int i = 0; i < nn; ++i) f.rmu[i] = a.rmu[i], f.wmu[i] = a.wmu[i];
      e = hd::launch_beer_surface(nn, f, stream);
      if (e == hipSuccess) {
        hd::BeerRayBwdArgs r{};
        r.prop = in->prop;
        r.albedo = in->albedo;
        r.fisot = in->fisot;
        r.planckv = planck_q;
        r.xsurf = seed_q;
        r.umu = rays->umu;
        r.cot = kcot;
        r.seed = seed_q;
        r.gb = gb_q;
        r.gtau = g->gtau;
        r.g_albedo = g->g_albedo;
        r.g_fbeam = g->g_fbeam;
        r.g_umu0 = g->g_umu0;
        r.g_fisot = g->g_fisot;
        r.status = status;
        r.anyerr = ctx->anyerr;
        r.s0 = s0;
        r.nsc = nsc;
        r.ncol = in->ncol;
        r.nlyr = nlyr;
        r.nprop = cfg->nprop;
        r.nray = rays->nray;
        r.per_column = rays->per_column;
        r.alpha = rays->alpha;
        e = hd::launch_beer_rays_bwd(r, stream);
      }
      if (e == hipSuccess) {
        a.seed = seed_q;
        e = hd::launch_beer_surface_bwd(nn, a, stream);
      }
    }
    if (e == hipSuccess && planck && (g->gtemf || g->g_btemp || g->g_ttemp || g->g_temis)) {
      hd::BeerPlanckBwdArgs pb{};
      pb.temf = in->temf;
      pb.btemp = in->btemp;
      pb.ttemp = in->ttemp;
      pb.temis = in->temis;
      pb.wlo = in->wave_lower;
      pb.whi = in->wave_upper;
      pb.planckv = planck_q;
      pb.gb = gb_q;
      pb.gtemf = g->gtemf;
      pb.g_btemp = g->g_btemp;
      pb.g_ttemp = g->g_ttemp;
      pb.g_temis = g->g_temis;
      pb.s0 = s0;
      pb.nsc = nsc;
      pb.ncol = in->ncol;
      pb.nlyr = nlyr;
      e = hd::launch_beer_planck_bwd(pb, stream);
    }
    if (e != hipSuccess)
      return fail(ctx, HD_EHIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  }
  return HD_OK;
}

}  // namespace

extern "C" {

int hd_beer_flux(hd_context* ctx, const hd_config* cfg, const hd_inputs* in, double* flux,
                 int* status, void* stream) {
  return solve_entry(
      ctx, "hd_beer_flux", in, status, stream,
      [&] { return validate(ctx, cfg, in, flux, "hd_beer_flux"); },
      [&](int*& st, hipStream_t s) {
        return beer_enqueue(ctx, cfg, in, flux, nullptr, nullptr, st, s, "hd_beer_flux");
      });
}

int hd_beer_flux_band(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                      const hd_band* band, double* flux, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_beer_flux_band", in, status, stream,
      [&] {
        if (!band || !band->weight || !band->bflux)
          return fail(ctx, HD_EINVAL, "hd_beer_flux_band: band weights and bflux are required");
        return validate(ctx, cfg, in, flux, "hd_beer_flux_band", /*out_optional=*/true);
      },
      [&](int*& st, hipStream_t s) {
        return beer_enqueue(ctx, cfg, in, flux, band, nullptr, st, s, "hd_beer_flux_band");
      });
}

int hd_beer_rays(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                 const struct hd_beer_rays* rays, double* rad, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_beer_rays", in, status, stream,
      [&] {
        if (!rays) return fail(ctx, HD_EINVAL, "hd_beer_rays: null ray config");
        if (!rad && !rays->brad)
          return fail(ctx, HD_EINVAL, "hd_beer_rays: rad and brad both NULL: nothing to compute");
        if (rays->brad && !rays->weight)
          return fail(ctx, HD_EINVAL, "hd_beer_rays: brad needs weight");
        if (rays->nray < 1 || !rays->umu)
          return fail(ctx, HD_EINVAL, "hd_beer_rays: rays need nray >= 1 and umu");
        if (rays->per_column != 0 && rays->per_column != 1)
          return fail(ctx, HD_EINVAL, "hd_beer_rays: per_column=%d must be 0 or 1",
                      rays->per_column);
        if (!(rays->alpha >= 0.0) || !std::isfinite(rays->alpha))
          return fail(ctx, HD_EINVAL, "hd_beer_rays: alpha=%g must be finite and >= 0",
                      rays->alpha);
        return validate(ctx, cfg, in, rad, "hd_beer_rays", /*out_optional=*/true);
      },
      [&](int*& st, hipStream_t s) {
        return beer_enqueue(ctx, cfg, in, rad, nullptr, rays, st, s, "hd_beer_rays");
      });
}

int hd_beer_flux_bwd(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                     const hd_beer_cot* cot, const hd_beer_grads* g, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_beer_flux_bwd", in, status, stream,
      [&] { return beer_bwd_check(ctx, cfg, in, cot, g, "hd_beer_flux_bwd"); },
      [&](int*& st, hipStream_t s) {
        return beer_bwd_enqueue(ctx, cfg, in, nullptr, cot, g, st, s, "hd_beer_flux_bwd");
      });
}

int hd_beer_rays_bwd(hd_context* ctx, const hd_config* cfg, const hd_inputs* in,
                     const struct hd_beer_rays* rays, const hd_beer_cot* cot,
                     const hd_beer_grads* g, int* status, void* stream) {
  return solve_entry(
      ctx, "hd_beer_rays_bwd", in, status, stream,
      [&] {
        const char* who = "hd_beer_rays_bwd";
        if (!rays) return fail(ctx, HD_EINVAL, "%s: null ray config", who);
        if (rays->nray < 1 || !rays->umu)
          return fail(ctx, HD_EINVAL, "%s: rays need nray >= 1 and umu", who);
        if (rays->per_column != 0 && rays->per_column != 1)
          return fail(ctx, HD_EINVAL, "%s: per_column=%d must be 0 or 1", who, rays->per_column);
        if (!(rays->alpha >= 0.0) || !std::isfinite(rays->alpha))
          return fail(ctx, HD_EINVAL, "%s: alpha=%g must be finite and >= 0", who, rays->alpha);
        return beer_bwd_check(ctx, cfg, in, cot, g, who);
      },
      [&](int*& st, hipStream_t s) {
        return beer_bwd_enqueue(ctx, cfg, in, rays, cot, g, st, s, "hd_beer_rays_bwd");
      });
}

}  // extern "C"
