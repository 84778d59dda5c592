// erpl_sampling.hip — the sampling half of the C ABI (include/erpl_mc.h): the reference's legacy RandomState streams and
// its per-sample wind profiles on the host, and the AR(1) wind synthesis kernel.
#include <math.h>

#include "erpl_host.h"

// ------------------------------------------------------------------ legacy RandomState streams
// MT19937 seeded like numpy.random.RandomState(int) (init_genrand), 53-bit doubles and the polar
// gaussian with its one-value cache - the published algorithms of the generator the reference draws
// from (monte_carlo.py:157 `np.random.RandomState(i)`).  Host code; built without FMA contraction so
// that x1*x1 + x2*x2 rounds like the baseline x86-64 build of NumPy.
namespace {
struct LegacyRS {
  uint32_t key[624];
  int pos;
  bool has_gauss;
  double gauss;
  void seed(uint32_t s) {
    for (int i = 0; i < 624; ++i) { key[i] = s; s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)i + 1u; }
    pos = 624; has_gauss = false; gauss = 0.0;
  }
  void refill() {
    const uint32_t A = 0x9908b0dfu, UP = 0x80000000u, LO = 0x7fffffffu;
    int k = 0;
    for (; k < 624 - 397; ++k) { uint32_t y = (key[k] & UP) | (key[k + 1] & LO); key[k] = key[k + 397] ^ (y >> 1) ^ ((y & 1u) ? A : 0u); }
    for (; k < 623; ++k) { uint32_t y = (key[k] & UP) | (key[k + 1] & LO); key[k] = key[k + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? A : 0u); }
    uint32_t y = (key[623] & UP) | (key[0] & LO);
    key[623] = key[396] ^ (y >> 1) ^ ((y & 1u) ? A : 0u);
    pos = 0;
  }
  uint32_t next32() {
    if (pos == 624) refill();
    uint32_t y = key[pos++];
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
  }
  double next_double() {
    const uint32_t a = next32() >> 5, b = next32() >> 6;
    return (a * 67108864.0 + b) / 9007199254740992.0;
  }
  double next_gauss() {
    if (has_gauss) { const double g = gauss; has_gauss = false; gauss = 0.0; return g; }
    double x1, x2, r2;
    do {
      x1 = 2.0 * next_double() - 1.0;
      x2 = 2.0 * next_double() - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double f = legacy_gauss_scale(r2);
    gauss = f * x1; has_gauss = true;
    return f * x2;
  }
};
}  // namespace

extern "C" {

int erpl_mc_legacy_random_streams(const uint32_t* seeds, int64_t n, const uint8_t* ops, int32_t m,
                                  double* out, int32_t by_output, int32_t threads) {
  if (n < 0 || m < 0) return erpl_fail(ERPL_ERR_INVALID, "negative size");
  if (n == 0 || m == 0) return ERPL_OK;
  if (!seeds || !ops || !out) return erpl_fail(ERPL_ERR_INVALID, "NULL buffer");
  for (int32_t j = 0; j < m; ++j)
    if (ops[j] != ERPL_RS_GAUSS && ops[j] != ERPL_RS_DOUBLE) return erpl_fail(ERPL_ERR_INVALID, "unknown stream op %d", (int)ops[j]);
  const int nthr = host_threads(threads, n);   // at least 64 streams per thread
  run_threads(nthr, [&](int w) {
    LegacyRS rs;
    const int64_t lo = n * w / nthr, hi = n * (w + 1) / nthr;
    for (int64_t i = lo; i < hi; ++i) {
      rs.seed(seeds[i]);
      double* o = by_output ? out + i : out + i * (int64_t)m;
      const int64_t stride = by_output ? n : 1;
      for (int32_t j = 0; j < m; ++j) o[j * stride] = (ops[j] == ERPL_RS_GAUSS) ? rs.next_gauss() : rs.next_double();
    }
  });
  return ERPL_OK;
}

int erpl_mc_legacy_wind_profiles(const uint32_t* seeds, int64_t n, int32_t k, const double* sigma,
                                 const double* rho, const double* innov, const double* base,
                                 const double* mean_scale, const double* speed, const double* cdir,
                                 const double* sdir, double* wind, int32_t threads) {
  if (n < 0 || k < 0) return erpl_fail(ERPL_ERR_INVALID, "negative size");
  if (n == 0 || k == 0) return ERPL_OK;
  if (!seeds || !sigma || !rho || !innov || !wind) return erpl_fail(ERPL_ERR_INVALID, "NULL buffer");
  if (!base && (!mean_scale || !speed || !cdir || !sdir)) return erpl_fail(ERPL_ERR_INVALID, "NULL mean-wind inputs");
  const int nthr = host_threads(threads, n);
  run_threads(nthr, [&](int w) {
    LegacyRS rs;
    const int64_t lo = n * w / nthr, hi = n * (w + 1) / nthr;
    for (int64_t s = lo; s < hi; ++s) {
      rs.seed(seeds[s]);
      double* o = wind + s;   // element (i, c) at o[(i * 3 + c) * n]
      double pu, pv, pw;      // previous knot's values
      if (base) {             // environment.py:218-265
        pu = base[0] + (0.0 + sigma[0] * rs.next_gauss());
        pv = base[1] + (0.0 + sigma[0] * rs.next_gauss());
        pw = base[2] + (0.0 + (sigma[0] * 0.3) * rs.next_gauss());
        o[0] = pu; o[n] = pv; o[2 * n] = pw;
        for (int32_t i = 1; i < k; ++i) {
          const double* b0 = base + 3 * (i - 1);
          const double* b1 = base + 3 * i;
          const double tu = rho[i] * (pu - b0[0]) + (0.0 + innov[i] * rs.next_gauss());
          const double tv = rho[i] * (pv - b0[1]) + (0.0 + innov[i] * rs.next_gauss());
          const double tw = rho[i] * (pw - b0[2]) + (0.0 + (innov[i] * 0.3) * rs.next_gauss());
          pu = b1[0] + tu; pv = b1[1] + tv; pw = b1[2] + tw;
          o[(int64_t)(3 * i) * n] = pu; o[(int64_t)(3 * i + 1) * n] = pv; o[(int64_t)(3 * i + 2) * n] = pw;
        }
      } else {                // environment.py:125-200
        const double cd = cdir[s], sd = sdir[s], sp = speed[s];
        double m = sp * mean_scale[0];
        pu = m * cd + (0.0 + sigma[0] * rs.next_gauss());
        pv = m * sd + (0.0 + sigma[0] * rs.next_gauss());
        pw = 0.0 + (sigma[0] * 0.3) * rs.next_gauss();
        o[0] = pu; o[n] = pv; o[2 * n] = pw;
        for (int32_t i = 1; i < k; ++i) {
          const double m1 = sp * mean_scale[i];
          const double tu = rho[i] * (pu - m * cd) + (0.0 + innov[i] * rs.next_gauss());
          const double tv = rho[i] * (pv - m * sd) + (0.0 + innov[i] * rs.next_gauss());
          const double tw = rho[i] * pw + (0.0 + (innov[i] * 0.3) * rs.next_gauss());
          pu = m1 * cd + tu; pv = m1 * sd + tv; pw = tw;
          m = m1;
          o[(int64_t)(3 * i) * n] = pu; o[(int64_t)(3 * i + 1) * n] = pv; o[(int64_t)(3 * i + 2) * n] = pw;
        }
      }
    }
  });
  return ERPL_OK;
}

}  // extern "C"

namespace {
// AR(1) turbulence over the altitude knots + mean wind for n samples at once (environment.py:161-198 /
// :242-263 with caller-supplied standard normals): one thread per (component, sample), sequential over
// the k knots, every access coalesced along the sample index.  fp64 recursion whatever the output type.
template <typename OUT>
__global__ __launch_bounds__(256) void erpl_wind_ar1(const int64_t n, const int k, const double* __restrict__ g,
                                                     const double* __restrict__ sigma, const double* __restrict__ rho,
                                                     const double* __restrict__ innov, const double* __restrict__ base,
                                                     const double* __restrict__ scale, const double* __restrict__ mean_u,
                                                     const double* __restrict__ mean_v, OUT* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 3 * n) return;
  const int c = (int)(idx / n);
  const int64_t s = idx - (int64_t)c * n;
  const double comp = (c == 2) ? 0.3 : 1.0;   // vertical component: 30 % of the horizontal turbulence
  const double m = (c == 0) ? mean_u[s] : ((c == 1) ? mean_v[s] : 0.0);
  double t = 0.0;
  for (int i = 0; i < k; ++i) {
    const double z = g[(int64_t)(i * 3 + c) * n + s];
    t = (i == 0) ? (sigma[0] * comp) * z : rho[i] * t + (innov[i] * comp) * z;
    const double b = base ? base[i * 3 + c] : 0.0;
    out[(int64_t)(i * 3 + c) * n + s] = (OUT)((b + scale[i] * m) + t);
  }
}
}  // namespace

extern "C" {

int erpl_mc_synth_wind(erpl_ctx* c, int64_t n, int32_t k, const double* normals, const double* sigma, const double* rho,
                       const double* innov, const double* base, const double* scale, const double* mean_u,
                       const double* mean_v, void* wind, int32_t precision, void* stream) {
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (n < 0 || k < 0 || k > ERPL_MAX_WIND_KNOTS) return erpl_fail(ERPL_ERR_INVALID, "bad size (n=%lld k=%d)", (long long)n, k);
  if (n == 0 || k == 0) return ERPL_OK;
  if (!normals || !sigma || !rho || !innov || !scale || !mean_u || !mean_v || !wind) return erpl_fail(ERPL_ERR_INVALID, "NULL buffer");
  if (precision != ERPL_PREC_F64 && precision != ERPL_PREC_F32 && precision != ERPL_PREC_F64_FAST)
    return erpl_fail(ERPL_ERR_INVALID, "unknown precision %d", precision);
  HIP_TRY(hipSetDevice(c->device));
  const int block = 256;
  const int64_t grid = (3 * n + block - 1) / block;
  if (precision == ERPL_PREC_F32)
    hipLaunchKernelGGL(erpl_wind_ar1<float>, dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, n, (int)k, normals, sigma,
                       rho, innov, base, scale, mean_u, mean_v, (float*)wind);
  else
    hipLaunchKernelGGL(erpl_wind_ar1<double>, dim3((unsigned)grid), dim3(block), 0, (hipStream_t)stream, n, (int)k, normals, sigma,
                       rho, innov, base, scale, mean_u, mean_v, (double*)wind);
  HIP_TRY(hipGetLastError());
  return ERPL_OK;
}

}  // extern "C"
