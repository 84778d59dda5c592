// erpl_legacy_device.hip — the legacy RandomState streams and the per-sample wind tables of erpl_sampling.hip drawn on the
// device, bit for bit: erpl_mc_legacy_random_streams_device and erpl_mc_legacy_wind_profiles_device.  LegacyRS in
// erpl_sampling.hip is the specification.
//
// Everything in the generator is integer or exactly rounded arithmetic except the libm log inside the scale
// f = sqrt(-2 log(r2) / r2) of an accepted pair: glibc's log is not correctly rounded, so only the host's own libm
// returns the host's bits.  Hence three phases per tile of samples:
//
//   draw    (device, one lane per stream)  init_genrand, twist, temper, the 53-bit doubles and the polar rejection loop.
//           Every stream consumes its words in order and two at a time (a double takes two words, a try four, a cached
//           normal none, and 624 is even), so ALL lanes of a tile are at the same double of the same 624-word block at
//           the same time: the state is a structure of arrays key[624][tile], seeded, twisted and read coalesced, and
//           a lane differs from its neighbours only in what it does with a double - which item of the stream it is
//           at, and whether it holds the first half of a try (a try may straddle a refill: x1 waits in a register).
//           The doubles of ERPL_RS_DOUBLE outputs go straight to `out`; an accepted pair leaves x1, x2 and r2 in the
//           workspace as [pair][sample].  The number of pairs is fixed by `ops`.
//   scale   (host)  r2 comes down to pinned memory, legacy_gauss_scale (erpl_host.h: the expression LegacyRS uses)
//           turns it into f on `threads` host threads, f goes back up.
//   finish  (device)  the normals f * x2 and f * x1, one rounded product each: written to out[m][n], or fed to the
//           AR(1) recursion of erpl_mc_legacy_wind_profiles, expression for expression.
//
// x1 and x2 stay in the workspace between draw and finish (24 bytes per pair next to the 2 496 bytes of state; the
// finish kernels are then plain element-wise passes).  The workspace holds one tile of states and two sets of pairs:
// while the host scales tile t the device draws tile t + 1, all on the caller's stream.  The tile is a function of the
// number of pairs alone and no value depends on it.  The rejection loop is bounded (kMaxTries per pair); a stream that
// hits the bound reports its sample and the call fails.  No kernel waits on another wave.
// Built without FMA contraction like every unit but the kernel units: x1*x1 + x2*x2 and the AR(1) expressions round as
// the host versions do.
#include <string.h>

#include <algorithm>

#include "erpl_host.h"

namespace {

constexpr int kBlock = 64;            // one wave per workgroup: a tile of 16 384 streams reaches every CU
constexpr int kMaxTries = 4096;       // per pair; a try is rejected with probability 1 - pi/4
constexpr int64_t kTile = 16384;      // streams per tile, less where a stream has many pairs (kPairBytes per set)
constexpr size_t kPairBytes = (size_t)64 << 20;
constexpr unsigned long long kNoSample = ~0ull;

struct DrawArgs {
  const uint32_t* seeds;   // [n]
  int64_t lo, n;           // the tile is samples lo .. lo + tn - 1
  int tn;
  const int32_t* items;    // what consumes doubles, in stream order: j >= 0 = the double of output j, < 0 = a pair
  int n_items;
  uint32_t* key;           // [624][tn]
  double *x1, *x2, *r2;    // [pairs][tn]
  double* out;             // [m][n] (doubles only; NULL for the wind tables)
  unsigned long long* bad; // lowest sample that ran out of tries
};

__device__ __forceinline__ uint32_t temper(uint32_t y) {
  y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
  return y;
}

__global__ __launch_bounds__(kBlock) void erpl_legacy_draw(const DrawArgs a) {
  const int l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= a.tn) return;
  const size_t ts = (size_t)a.tn;
  uint32_t* key = a.key + l;   // word i of this lane's state at key[i * ts]
  uint32_t s = a.seeds[a.lo + l];
  for (int i = 0; i < 624; ++i) { key[i * ts] = s; s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i + 1u; }
  int it = 0, pair = 0, tries = 0;
  bool have = false;
  double x1 = 0.0;
  while (it < a.n_items) {
    {   // LegacyRS::refill
      const uint32_t A = 0x9908b0dfu, UP = 0x80000000u, LO = 0x7fffffffu;
      int k = 0;
      for (; k < 624 - 397; ++k) { const uint32_t y = (key[k * ts] & UP) | (key[(k + 1) * ts] & LO); key[k * ts] = key[(k + 397) * ts] ^ (y >> 1) ^ ((y & 1u) ? A : 0u); }
      for (; k < 623; ++k) { const uint32_t y = (key[k * ts] & UP) | (key[(k + 1) * ts] & LO); key[k * ts] = key[(k + (397 - 624)) * ts] ^ (y >> 1) ^ ((y & 1u) ? A : 0u); }
      const uint32_t y = (key[623 * ts] & UP) | (key[0] & LO);
      key[623 * ts] = key[396 * ts] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    }
    for (int d = 0; d < 312 && it < a.n_items; ++d) {
      const uint32_t wa = temper(key[(2 * d) * ts]) >> 5, wb = temper(key[(2 * d + 1) * ts]) >> 6;
      const double v = (wa * 67108864.0 + wb) * 0x1.0p-53;   // (a 2^26 + b) / 2^53: exact
      const int item = a.items[it];
      if (item >= 0) {
        a.out[(int64_t)item * a.n + a.lo + l] = v;
        ++it;
      } else if (!have) {
        x1 = 2.0 * v - 1.0;
        have = true;
      } else {
        const double x2 = 2.0 * v - 1.0;
        const double r2 = x1 * x1 + x2 * x2;
        have = false;
        if (!(r2 >= 1.0 || r2 == 0.0)) {
          const size_t at = (size_t)pair * ts + l;
          a.x1[at] = x1; a.x2[at] = x2; a.r2[at] = r2;
          ++pair; ++it; tries = 0;
        } else if (++tries >= kMaxTries) {
          atomicMin(a.bad, (unsigned long long)(a.lo + l));
          it = a.n_items;
        }
      }
    }
  }
}

// out[j][lo + l] = normal number g of the stream = f * x2 (g even) or f * x1 (the cached one) of pair g / 2
__global__ __launch_bounds__(256) void erpl_legacy_finish_streams(const int64_t lo, const int64_t n, const int tn,
                                                                   const int32_t* __restrict__ rowmap,
                                                                   const double* __restrict__ x1, const double* __restrict__ x2,
                                                                   const double* __restrict__ f, double* __restrict__ out) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  const int g = rowmap[blockIdx.y];   // < 0: a double, already in place
  if (l >= tn || g < 0) return;
  const size_t at = (size_t)(g >> 1) * (size_t)tn + l;
  out[(int64_t)blockIdx.y * n + lo + l] = f[at] * ((g & 1) ? x1[at] : x2[at]);
}

struct WindArgs {
  int64_t lo, n;
  int tn, k;
  const double *sigma, *rho, *innov, *base, *mean_scale;   // device copies of the host arrays; base or mean_scale is NULL
  const double *speed, *cdir, *sdir;                        // [n]
  const double *x1, *x2, *f;                                // [pairs][tn]
  double* wind;                                             // [k][3][n]
};

// the recursion of erpl_mc_legacy_wind_profiles, expression for expression (the 0.0 + ... terms turn -0.0 into +0.0)
__global__ __launch_bounds__(kBlock) void erpl_legacy_finish_wind(const WindArgs a) {
  const int l = blockIdx.x * kBlock + threadIdx.x;
  if (l >= a.tn) return;
  const size_t ts = (size_t)a.tn;
  const int64_t n = a.n;
  int g = 0;   // normals drawn so far
  auto next_gauss = [&]() {
    const size_t at = (size_t)(g >> 1) * ts + l;
    const double z = a.f[at] * ((g & 1) ? a.x1[at] : a.x2[at]);
    ++g;
    return z;
  };
  const double *sigma = a.sigma, *rho = a.rho, *innov = a.innov, *base = a.base, *mean_scale = a.mean_scale;
  double* o = a.wind + a.lo + l;   // element (i, c) at o[(i * 3 + c) * n]
  double pu, pv, pw;
  if (base) {
    pu = base[0] + (0.0 + sigma[0] * next_gauss());
    pv = base[1] + (0.0 + sigma[0] * next_gauss());
    pw = base[2] + (0.0 + (sigma[0] * 0.3) * next_gauss());
    o[0] = pu; o[n] = pv; o[2 * n] = pw;
    for (int i = 1; i < a.k; ++i) {
      const double* b0 = base + 3 * (i - 1);
      const double* b1 = base + 3 * i;
      const double tu = rho[i] * (pu - b0[0]) + (0.0 + innov[i] * next_gauss());
      const double tv = rho[i] * (pv - b0[1]) + (0.0 + innov[i] * next_gauss());
      const double tw = rho[i] * (pw - b0[2]) + (0.0 + (innov[i] * 0.3) * next_gauss());
      pu = b1[0] + tu; pv = b1[1] + tv; pw = b1[2] + tw;
      o[(int64_t)(3 * i) * n] = pu; o[(int64_t)(3 * i + 1) * n] = pv; o[(int64_t)(3 * i + 2) * n] = pw;
    }
  } else {
    const double cd = a.cdir[a.lo + l], sd = a.sdir[a.lo + l], sp = a.speed[a.lo + l];
    double m = sp * mean_scale[0];
    pu = m * cd + (0.0 + sigma[0] * next_gauss());
    pv = m * sd + (0.0 + sigma[0] * next_gauss());
    pw = 0.0 + (sigma[0] * 0.3) * next_gauss();
    o[0] = pu; o[n] = pv; o[2 * n] = pw;
    for (int i = 1; i < a.k; ++i) {
      const double m1 = sp * mean_scale[i];
      const double tu = rho[i] * (pu - m * cd) + (0.0 + innov[i] * next_gauss());
      const double tv = rho[i] * (pv - m * sd) + (0.0 + innov[i] * next_gauss());
      const double tw = rho[i] * pw + (0.0 + (innov[i] * 0.3) * next_gauss());
      pu = m1 * cd + tu; pv = m1 * sd + tv; pw = tw;
      m = m1;
      o[(int64_t)(3 * i) * n] = pu; o[(int64_t)(3 * i + 1) * n] = pv; o[(int64_t)(3 * i + 2) * n] = pw;
    }
  }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int grow_pinned(erpl_ctx* c, size_t bytes) {
  if (bytes <= c->legacy_pin_cap) return ERPL_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (c->legacy_pin) (void)hipHostFree(c->legacy_pin);
  c->legacy_pin = nullptr; c->legacy_pin_cap = 0;
  HIP_TRY(hipHostMalloc((void**)&c->legacy_pin, bytes, hipHostMallocDefault));
  c->legacy_pin_cap = bytes;
  return ERPL_OK;
}

// What one call hands to the three phases.  `items` / `n_pairs` describe the stream; the small host tables
// (`tables`, `table_bytes`: the items first) are copied to the workspace once; `finish` launches the tile's last phase.
struct Plan {
  const uint32_t* seeds;
  int64_t n;
  int n_items, n_pairs;
  const void* tables;
  size_t table_bytes;
  double* out;   // the draw phase's target for doubles, or NULL
  // (device copy of the tables, tile start, tile size, x1, x2, f)
  std::function<void(const char*, int64_t, int, const double*, const double*, const double*)> finish;
};

int run_plan(erpl_ctx* c, const Plan& p, int32_t threads, hipStream_t st) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t P = (size_t)p.n_pairs;
  int64_t tile = std::min<int64_t>(kTile, (int64_t)(kPairBytes / (24 * std::max<size_t>(P, 1)))) & ~(int64_t)255;
  tile = std::min(std::max<int64_t>(tile, 256), p.n);
  const size_t T = (size_t)tile;
  // device: [bad 256][tables][key 624 T u32][set 0: x1, x2, r2/f  P T doubles each][set 1]; pinned: [bad per set 256][tables][set 0: r2/f][set 1]
  const size_t off_tab = 256, off_key = off_tab + align256(p.table_bytes), off_set = off_key + align256(624 * T * 4);
  const size_t arr = align256(P * T * 8);
  const size_t pin_set = off_tab + align256(p.table_bytes);
  ERPL_TRY(erpl_grow(c->legacy_buf, c->legacy_cap, off_set + 6 * arr));
  ERPL_TRY(grow_pinned(c, pin_set + 2 * arr));
  for (hipEvent_t& e : c->legacy_ev)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  char *dev = c->legacy_buf, *pin = c->legacy_pin;
  unsigned long long* d_bad = (unsigned long long*)dev;
  HIP_TRY(hipMemsetAsync(d_bad, 0xff, sizeof(*d_bad), st));
  memcpy(pin + off_tab, p.tables, p.table_bytes);
  HIP_TRY(hipMemcpyAsync(dev + off_tab, pin + off_tab, p.table_bytes, hipMemcpyHostToDevice, st));
  auto set_arr = [&](char* base0, size_t first, int set, int which) { return (double*)(base0 + first + ((size_t)set * 3 + which) * arr); };
  auto pin_r2 = [&](int set) { return (double*)(pin + pin_set + (size_t)set * arr); };
  auto pin_bad = [&](int set) { return (unsigned long long*)(pin + 128 * set); };

  const int64_t ntiles = (p.n + tile - 1) / tile;
  auto draw = [&](int64_t t) -> int {
    const int set = (int)(t & 1);
    DrawArgs a;
    a.seeds = p.seeds; a.lo = t * tile; a.n = p.n; a.tn = (int)std::min<int64_t>(tile, p.n - a.lo);
    a.items = (const int32_t*)(dev + off_tab); a.n_items = p.n_items;
    a.key = (uint32_t*)(dev + off_key);
    a.x1 = set_arr(dev, off_set, set, 0); a.x2 = set_arr(dev, off_set, set, 1); a.r2 = set_arr(dev, off_set, set, 2);
    a.out = p.out; a.bad = d_bad;
    hipLaunchKernelGGL(erpl_legacy_draw, dim3((a.tn + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (P) {
      HIP_TRY(hipMemcpyAsync(pin_r2(set), a.r2, P * (size_t)a.tn * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(pin_bad(set), d_bad, sizeof(*d_bad), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipEventRecord(c->legacy_ev[set], st));
    }
    return ERPL_OK;
  };
  ERPL_TRY(draw(0));
  for (int64_t t = 0; t < ntiles; ++t) {
    if (t + 1 < ntiles) ERPL_TRY(draw(t + 1));   // runs while the host scales tile t
    if (!P) continue;
    const int set = (int)(t & 1);
    const int64_t lo = t * tile;
    const int tn = (int)std::min<int64_t>(tile, p.n - lo);
    HIP_TRY(hipEventSynchronize(c->legacy_ev[set]));
    if (*pin_bad(set) != kNoSample) {
      const unsigned long long s = *pin_bad(set);
      (void)hipStreamSynchronize(st);
      return erpl_fail(ERPL_ERR_INVALID, "the stream of sample %llu rejected %d tries of one pair in a row", s, kMaxTries);
    }
    double* r = pin_r2(set);
    const int64_t total = (int64_t)P * tn;
    const int nthr = host_threads(threads, total);
    run_threads(nthr, [&](int w) {
      for (int64_t i = total * w / nthr, hi = total * (w + 1) / nthr; i < hi; ++i) r[i] = legacy_gauss_scale(r[i]);
    });
    double* d_f = set_arr(dev, off_set, set, 2);
    HIP_TRY(hipMemcpyAsync(d_f, r, (size_t)total * 8, hipMemcpyHostToDevice, st));
    p.finish(dev + off_tab, lo, tn, set_arr(dev, off_set, set, 0), set_arr(dev, off_set, set, 1), d_f);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(st));
  return ERPL_OK;
}

}  // namespace

extern "C" {

int erpl_mc_legacy_random_streams_device(erpl_ctx* c, const uint32_t* seeds, int64_t n, const uint8_t* ops, int32_t m,
                                         double* out, int32_t threads, void* stream) {
  if (n < 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld is negative", (long long)n);
  if (m < 0) return erpl_fail(ERPL_ERR_INVALID, "m = %d is negative", m);
  if (n >= (1ll << 31)) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: at most 2^31 - 1 streams per call", (long long)n);
  if (m > ERPL_LEGACY_DEVICE_MAX_OUTPUTS)
    return erpl_fail(ERPL_ERR_INVALID, "m = %d exceeds ERPL_LEGACY_DEVICE_MAX_OUTPUTS (%d)", m, ERPL_LEGACY_DEVICE_MAX_OUTPUTS);
  if (n == 0 || m == 0) return ERPL_OK;
  if (!seeds) return erpl_fail(ERPL_ERR_INVALID, "seeds is NULL");
  if (!ops) return erpl_fail(ERPL_ERR_INVALID, "ops is NULL");
  if (!out) return erpl_fail(ERPL_ERR_INVALID, "out is NULL");
  for (int32_t j = 0; j < m; ++j)
    if (ops[j] != ERPL_RS_GAUSS && ops[j] != ERPL_RS_DOUBLE)
      return erpl_fail(ERPL_ERR_INVALID, "ops[%d] = %d: unknown stream op", j, (int)ops[j]);
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  // items (what consumes doubles, in order) and, per output, which normal of the stream it is: every second
  // ERPL_RS_GAUSS takes the cached half of the pair before it and consumes nothing
  std::vector<int32_t> tab(2 * (size_t)m);
  int32_t *items = tab.data(), *rowmap = items + m;
  int n_items = 0, g = 0;
  for (int32_t j = 0; j < m; ++j) {
    if (ops[j] == ERPL_RS_DOUBLE) { items[n_items++] = j; rowmap[j] = -1; continue; }
    if ((g & 1) == 0) items[n_items++] = -1;
    rowmap[j] = g++;
  }
  for (int i = n_items; i < m; ++i) items[i] = -1;
  Plan p;
  p.seeds = seeds; p.n = n; p.n_items = n_items; p.n_pairs = (g + 1) / 2;
  p.tables = tab.data(); p.table_bytes = tab.size() * sizeof(int32_t);
  p.out = out;
  hipStream_t st = (hipStream_t)stream;
  p.finish = [&](const char* tables, int64_t lo, int tn, const double* x1, const double* x2, const double* f) {
    hipLaunchKernelGGL(erpl_legacy_finish_streams, dim3((tn + 255) / 256, m), dim3(256), 0, st, lo, n, tn,
                       (const int32_t*)tables + m, x1, x2, f, out);
  };
  return run_plan(c, p, threads, st);
}

int erpl_mc_legacy_wind_profiles_device(erpl_ctx* c, const uint32_t* seeds, int64_t n, int32_t k, const double* sigma,
                                        const double* rho, const double* innov, const double* base,
                                        const double* mean_scale, const double* speed, const double* cdir,
                                        const double* sdir, double* wind, int32_t threads, void* stream) {
  if (n < 0) return erpl_fail(ERPL_ERR_INVALID, "n = %lld is negative", (long long)n);
  if (k < 0) return erpl_fail(ERPL_ERR_INVALID, "k = %d is negative", k);
  if (n >= (1ll << 31)) return erpl_fail(ERPL_ERR_INVALID, "n = %lld: at most 2^31 - 1 samples per call", (long long)n);
  if (k > ERPL_MAX_WIND_KNOTS) return erpl_fail(ERPL_ERR_INVALID, "k = %d exceeds ERPL_MAX_WIND_KNOTS (%d)", k, ERPL_MAX_WIND_KNOTS);
  if (n == 0 || k == 0) return ERPL_OK;
  if (!seeds) return erpl_fail(ERPL_ERR_INVALID, "seeds is NULL");
  if (!sigma) return erpl_fail(ERPL_ERR_INVALID, "sigma is NULL");
  if (!rho) return erpl_fail(ERPL_ERR_INVALID, "rho is NULL");
  if (!innov) return erpl_fail(ERPL_ERR_INVALID, "innov is NULL");
  if (!wind) return erpl_fail(ERPL_ERR_INVALID, "wind is NULL");
  if (!base) {
    if (!mean_scale) return erpl_fail(ERPL_ERR_INVALID, "mean_scale is NULL (and so is base)");
    if (!speed) return erpl_fail(ERPL_ERR_INVALID, "speed is NULL (and so is base)");
    if (!cdir) return erpl_fail(ERPL_ERR_INVALID, "cdir is NULL (and so is base)");
    if (!sdir) return erpl_fail(ERPL_ERR_INVALID, "sdir is NULL (and so is base)");
  }
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "ctx is NULL");
  // 3 k normals per stream and nothing else: ceil(3 k / 2) pairs.  Tables: the items, then sigma, rho, innov and
  // base [k][3] or mean_scale [k], 8-byte aligned behind an even number of items.
  const int n_pairs = (3 * k + 1) / 2, n_items = n_pairs + (n_pairs & 1);
  const size_t uk = (size_t)k, tail = base ? 3 * uk : uk;
  std::vector<double> tab(n_items / 2 + 3 * uk + tail);
  memset(tab.data(), 0xff, (size_t)n_items * sizeof(int32_t));   // every item a pair
  double* t_sigma = tab.data() + n_items / 2;
  memcpy(t_sigma, sigma, uk * 8);
  memcpy(t_sigma + uk, rho, uk * 8);
  memcpy(t_sigma + 2 * uk, innov, uk * 8);
  memcpy(t_sigma + 3 * uk, base ? base : mean_scale, tail * 8);
  Plan p;
  p.seeds = seeds; p.n = n; p.n_items = n_pairs; p.n_pairs = n_pairs;
  p.tables = tab.data(); p.table_bytes = tab.size() * sizeof(double);
  p.out = nullptr;
  hipStream_t st = (hipStream_t)stream;
  p.finish = [&](const char* tables, int64_t lo, int tn, const double* x1, const double* x2, const double* f) {
    WindArgs a;
    a.lo = lo; a.n = n; a.tn = tn; a.k = k;
    a.sigma = (const double*)tables + n_items / 2; a.rho = a.sigma + uk; a.innov = a.rho + uk;
    a.base = base ? a.innov + uk : nullptr;
    a.mean_scale = base ? nullptr : a.innov + uk;
    a.speed = speed; a.cdir = cdir; a.sdir = sdir;
    a.x1 = x1; a.x2 = x2; a.f = f; a.wind = wind;
    hipLaunchKernelGGL(erpl_legacy_finish_wind, dim3((tn + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
  };
  return run_plan(c, p, threads, st);
}

}  // extern "C"
