// erpl_qmc.hip — erpl_mc_qmc of the C ABI (include/erpl_mc.h): the primitives of a run as a scrambled Sobol' design on the
// rows that have a dimension, padded with the rows of erpl_mc_design on those that have none.  The values are those of
// erpl_qmc.h and erpl_design.h, here for the device (erpl_qmc_fill) and for the host (erpl_mc_qmc_host); built without FMA
// contraction, so that x' + u rounds alike on both.
#include "erpl_host.h"

#include <mutex>

#include "erpl_qmc.h"

namespace {
constexpr int kQmcBlock = 256;
constexpr int kQmcRows = 512;     // rows of one launch: what travels by value stays near 1 KB

// What the kernel takes by value: the design, the window, and per row of the launch its dimension and whether it is normal.
struct ErplQmcArgs {
  uint64_t seed;
  int64_t first, count, ld;
  uint32_t n, m, b, first_row;    // first_row: the GLOBAL row of the launch's row 0
  int32_t scramble, pad;
  uint32_t normal[kQmcRows / 32];
  uint32_t dims[kQmcRows / 2];    // two int16 per word, the even row in the low half: a word is a scalar load
};

// One thread per (row, column), columns fastest: a wave stores 512 contiguous bytes.  blockIdx.y is the row of the launch, so
// row, dimension and kind are the workgroup's own: the dimension and its 32 direction words come through scalar loads (the
// index is uniform) and stay in scalar registers.  Its 256 columns lie in up to 256 replicates (a border, or
// a block below 256): thread t draws the keys of the workgroup's t-th replicate once, into LDS, and every lane reads those
// of its own replicate (a broadcast where there is one).  A pad row keeps the six round keys of erpl_mc_design there, a
// Sobol' row its two scramble keys.  n < 2^31: a column, a replicate and a local index fit 32 bits; only the offset into
// `out` needs 64.  No atomics: the flag is a plain store of 1, whoever gets there.
__global__ __launch_bounds__(kQmcBlock) void erpl_qmc_fill(const ErplQmcArgs a, const uint32_t* __restrict__ V,
                                                           double* __restrict__ out, int* flag) {
  __shared__ uint32_t keys[kQmcBlock * 6];
  const uint32_t row = blockIdx.y, g = a.first_row + row;
  const int32_t d = (int16_t)(a.dims[row >> 1] >> ((row & 1u) * 16u));
  const bool sobol = d >= 0;
  const bool keyed = sobol ? a.scramble == ERPL_QMC_OWEN : a.pad != ERPL_DESIGN_RANDOM;
  const int64_t c0 = (int64_t)blockIdx.x * kQmcBlock;
  const int64_t c = c0 + threadIdx.x;
  uint32_t rho0 = 0;
  if (keyed) {
    const int64_t c1 = c0 + kQmcBlock - 1 < a.count - 1 ? c0 + kQmcBlock - 1 : a.count - 1;
    rho0 = (uint32_t)(a.first + c0) / a.m;
    const uint32_t n_rep = (uint32_t)(a.first + c1) / a.m - rho0 + 1u;   // <= 256: the workgroup has 256 columns
    if (threadIdx.x < n_rep) {
      if (sobol) {
        erpl_qmc_keys(a.seed, g, rho0 + threadIdx.x, &keys[threadIdx.x * 6], &keys[threadIdx.x * 6 + 1]);
      } else {
        const ErplDesignKeys K = erpl_design_keys(a.seed, g, rho0 + threadIdx.x);
#pragma unroll
        for (int j = 0; j < 6; ++j) keys[threadIdx.x * 6 + j] = K.k[j];
      }
    }
    __syncthreads();
  }
  if (c >= a.count) return;
  const uint32_t i = (uint32_t)(a.first + c);
  uint32_t rho = 0, l = i;
  if (a.m != a.n) { rho = i / a.m; l = i - rho * a.m; }
  const bool normal = (a.normal[row >> 5] >> (row & 31u)) & 1u;
  double v;
  if (sobol) {
    uint32_t dir[ERPL_QMC_BITS];
    const uint32_t* vd = V + (uint32_t)d * ERPL_QMC_BITS;
#pragma unroll
    for (int j = 0; j < ERPL_QMC_BITS; ++j) dir[j] = vd[j];
    uint32_t k0 = 0, k1 = 0;
    if (keyed) { k0 = keys[(rho - rho0) * 6]; k1 = keys[(rho - rho0) * 6 + 1]; }
    v = erpl_qmc_value(a.seed, a.scramble, normal, g, i, dir, l, k0, k1);
  } else {
    uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (keyed) {
#pragma unroll
      for (int j = 0; j < 6; ++j) k[j] = keys[(rho - rho0) * 6 + j];
    }
    bool capped = false;
    v = erpl_design_value(a.seed, a.pad, normal, g, i, k, a.b, a.m, l, &capped);
    if (capped) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  out[(int64_t)row * a.ld + c] = v;
}

// V[ERPL_QMC_MAX_DIMS][32] on the host, expanded once per process
const uint32_t* qmc_table() {
  static std::vector<uint32_t> V;
  static bool ok = false;
  static std::once_flag once;
  std::call_once(once, [] {
    V.resize((size_t)ERPL_QMC_MAX_DIMS * ERPL_QMC_BITS);
    ok = erpl_qmc_expand(V.data());
  });
  return ok ? V.data() : nullptr;
}

int32_t dim_of(const erpl_qmc_spec* s, const int32_t* dims, int32_t r) {
  if (dims) return dims[r];
  const int32_t g = s->first_row + r;
  return g < ERPL_QMC_MAX_DIMS ? g : -1;
}

// the refusals of erpl_mc_qmc and erpl_mc_qmc_host, in the order of the header
int qmc_check(const erpl_qmc_spec* s, const uint8_t* kinds, const int32_t* dims, int64_t first, int64_t count, const double* out,
              int64_t ld) {
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!kinds) return erpl_fail(ERPL_ERR_INVALID, "kinds is NULL");
  if (!out) return erpl_fail(ERPL_ERR_INVALID, "out is NULL");
  if (s->scramble != ERPL_QMC_RAW && s->scramble != ERPL_QMC_OWEN) return erpl_fail(ERPL_ERR_INVALID, "unknown scramble %d", s->scramble);
  if (s->pad != ERPL_DESIGN_RANDOM && s->pad != ERPL_DESIGN_LHS)
    return erpl_fail(ERPL_ERR_INVALID, "pad = %d is neither ERPL_DESIGN_RANDOM nor ERPL_DESIGN_LHS", s->pad);
  if (s->rows < 1 || s->first_row < 0 || (int64_t)s->first_row + s->rows > ERPL_DESIGN_MAX_ROWS)
    return erpl_fail(ERPL_ERR_INVALID, "rows = %d, first_row = %d outside 1 <= rows, 0 <= first_row, first_row + rows <= %d", s->rows,
                     s->first_row, ERPL_DESIGN_MAX_ROWS);
  if (s->n < 1 || s->n >= ((int64_t)1 << 31)) return erpl_fail(ERPL_ERR_INVALID, "n = %lld outside 1 .. 2^31 - 1", (long long)s->n);
  if (s->block < 0 || s->block > s->n || (s->block > 0 && s->n % s->block != 0))
    return erpl_fail(ERPL_ERR_INVALID, "block = %lld is negative, above n or does not divide n = %lld", (long long)s->block, (long long)s->n);
  if (first < 0) return erpl_fail(ERPL_ERR_INVALID, "first = %lld is negative", (long long)first);
  if (count < 0) return erpl_fail(ERPL_ERR_INVALID, "count = %lld is negative", (long long)count);
  if (first > s->n || count > s->n - first)
    return erpl_fail(ERPL_ERR_INVALID, "first + count = %lld + %lld exceeds n = %lld", (long long)first, (long long)count, (long long)s->n);
  if (ld < count) return erpl_fail(ERPL_ERR_INVALID, "ld = %lld is below count = %lld", (long long)ld, (long long)count);
  for (int32_t r = 0; r < s->rows; ++r)
    if (kinds[r] != ERPL_DESIGN_UNIFORM && kinds[r] != ERPL_DESIGN_NORMAL)
      return erpl_fail(ERPL_ERR_INVALID, "kinds[%d] = %d is neither ERPL_DESIGN_UNIFORM nor ERPL_DESIGN_NORMAL", r, (int)kinds[r]);
  for (int32_t r = 0; r < s->rows; ++r) {
    const int32_t d = dim_of(s, dims, r);
    if (d < -1 || d >= ERPL_QMC_MAX_DIMS)
      return erpl_fail(ERPL_ERR_INVALID, "dims[%d] = %d outside -1 .. %d", r, d, ERPL_QMC_MAX_DIMS - 1);
  }
  int32_t owner[ERPL_QMC_MAX_DIMS];
  for (int32_t& o : owner) o = -1;
  for (int32_t r = 0; r < s->rows; ++r) {
    const int32_t d = dim_of(s, dims, r);
    if (d < 0) continue;
    if (owner[d] >= 0) return erpl_fail(ERPL_ERR_INVALID, "dims[%d] = dims[%d] = %d: two rows of one call on the same dimension", owner[d], r, d);
    owner[d] = r;
  }
  return ERPL_OK;
}

int qmc_no_table() { return erpl_fail(ERPL_ERR_INTERNAL, "erpl_mc_qmc: the table of direction numbers does not expand to %d dimensions", ERPL_QMC_MAX_DIMS); }
}  // namespace

extern "C" {

int erpl_mc_qmc_defaults(erpl_qmc_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  *spec = erpl_qmc_spec{};
  spec->rows = 1;
  spec->scramble = ERPL_QMC_OWEN;
  spec->pad = ERPL_DESIGN_RANDOM;
  spec->n = 1;
  return ERPL_OK;
}

int erpl_mc_qmc(erpl_ctx* c, const erpl_qmc_spec* spec, const uint8_t* kinds, const int32_t* dims, int64_t first, int64_t count,
                double* out, int64_t ld, void* stream) {
  ERPL_TRY(qmc_check(spec, kinds, dims, first, count, out, ld));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (count == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(erpl_design_flag_init(c));
  if (!c->qmc_v) {
    const uint32_t* V = qmc_table();
    if (!V) return qmc_no_table();
    const size_t bytes = (size_t)ERPL_QMC_MAX_DIMS * ERPL_QMC_BITS * sizeof(uint32_t);
    uint32_t* dv = nullptr;
    HIP_TRY(hipMalloc((void**)&dv, bytes));
    const hipError_t e = hipMemcpy(dv, V, bytes, hipMemcpyHostToDevice);    // blocking: every later launch finds it there
    if (e != hipSuccess) { (void)hipFree(dv); return erpl_fail(ERPL_ERR_HIP, "hipMemcpy of the direction numbers: %s", hipGetErrorString(e)); }
    c->qmc_v = dv;
  }
  ErplQmcArgs a = {};
  a.seed = spec->seed;
  a.first = first; a.count = count; a.ld = ld;
  a.n = (uint32_t)spec->n;
  a.m = (uint32_t)(spec->block ? spec->block : spec->n);
  a.b = erpl_design_half_bits(a.m);
  a.scramble = spec->scramble;
  a.pad = spec->pad;
  const unsigned tiles = (unsigned)((count + kQmcBlock - 1) / kQmcBlock);
  for (int32_t r0 = 0; r0 < spec->rows; r0 += kQmcRows) {
    const int32_t rows = spec->rows - r0 < kQmcRows ? spec->rows - r0 : kQmcRows;
    a.first_row = (uint32_t)(spec->first_row + r0);
    for (uint32_t& w : a.normal) w = 0u;
    for (uint32_t& w : a.dims) w = 0u;
    for (int32_t r = 0; r < rows; ++r) {
      if (kinds[r0 + r] == ERPL_DESIGN_NORMAL) a.normal[r >> 5] |= 1u << (r & 31);
      a.dims[r >> 1] |= (uint32_t)(uint16_t)(int16_t)dim_of(spec, dims, r0 + r) << ((r & 1) * 16);
    }
    hipLaunchKernelGGL(erpl_qmc_fill, dim3(tiles, (unsigned)rows), dim3(kQmcBlock), 0, (hipStream_t)stream, a, c->qmc_v,
                       out + (int64_t)r0 * ld, c->design_flag);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->design_ev, (hipStream_t)stream));
  return ERPL_OK;
}

int erpl_mc_qmc_host(const erpl_qmc_spec* spec, const uint8_t* kinds, const int32_t* dims, int64_t first, int64_t count, double* out,
                     int64_t ld) {
  ERPL_TRY(qmc_check(spec, kinds, dims, first, count, out, ld));
  if (count == 0) return ERPL_OK;
  const uint32_t* V = qmc_table();
  if (!V) return qmc_no_table();
  const uint64_t seed = spec->seed;
  const uint32_t m = (uint32_t)(spec->block ? spec->block : spec->n), b = erpl_design_half_bits(m);
  const int scramble = spec->scramble, pad = spec->pad;
  const int nthr = host_threads(0, count);
  std::vector<char> capped(nthr, 0);
  run_threads(nthr, [&](int w) {
    const int64_t lo = count * w / nthr, hi = count * (w + 1) / nthr;
    for (int32_t r = 0; r < spec->rows; ++r) {
      const uint32_t g = (uint32_t)(spec->first_row + r);
      const int32_t d = dim_of(spec, dims, r);
      const bool normal = kinds[r] == ERPL_DESIGN_NORMAL;
      ErplDesignKeys K = {};
      uint32_t k0 = 0, k1 = 0;
      int64_t have = -1;    // the replicate the keys belong to
      for (int64_t c = lo; c < hi; ++c) {
        const uint32_t i = (uint32_t)(first + c), rho = i / m, l = i - rho * m;
        if (have != (int64_t)rho) {
          if (d >= 0 && scramble == ERPL_QMC_OWEN) erpl_qmc_keys(seed, g, rho, &k0, &k1);
          if (d < 0 && pad != ERPL_DESIGN_RANDOM) K = erpl_design_keys(seed, g, rho);
          have = rho;
        }
        if (d >= 0) {
          out[(int64_t)r * ld + c] = erpl_qmc_value(seed, scramble, normal, g, i, V + (size_t)d * ERPL_QMC_BITS, l, k0, k1);
        } else {
          bool cap = false;
          out[(int64_t)r * ld + c] = erpl_design_value(seed, pad, normal, g, i, K.k, b, m, l, &cap);
          if (cap) capped[w] = 1;
        }
      }
    }
  });
  for (char f : capped)
    if (f) return erpl_fail(ERPL_ERR_INTERNAL, "erpl_mc_qmc: a cycle walk reached %d trips; its values are NaN", ERPL_DESIGN_WALK_CAP);
  return ERPL_OK;
}

}  // extern "C"
