// erpl_design.hip — erpl_mc_design of the C ABI (include/erpl_mc.h): the primitives of a run as one counter-based design,
// independent draws or Latin hypercube samples.  The values are those of erpl_design.h, here for the device
// (erpl_design_fill) and for the host (erpl_mc_design_host); built without FMA contraction, so that s = pi + u and p = s / m
// round alike on both.
#include "erpl_host.h"

#include "erpl_design.h"

namespace {
constexpr int kDesignBlock = 256;

// What the kernel takes by value: the design, the window and one bit per row of the call (set: a normal row).
struct ErplDesignArgs {
  uint64_t seed;
  int64_t first, count, ld;
  uint32_t n, m, b, first_row;
  int32_t kind;
  uint32_t normal[ERPL_DESIGN_MAX_ROWS / 32];
};

// One thread per (row, column), columns fastest: a wave stores 512 contiguous bytes.  blockIdx.y is the row of the call, so
// row and kind are the workgroup's own, and its 256 columns lie in one replicate or, at a border or with a block below 256,
// in up to 256 of them: thread t draws the six round keys of the workgroup's t-th replicate once, into LDS, and every lane
// reads those of its own replicate (a broadcast where the workgroup has one).  n < 2^31: a global column, a replicate and a
// stratum fit 32 bits; only the offset into `out` needs 64 (rows x ld exceeds 2^32).
__global__ __launch_bounds__(kDesignBlock) void erpl_design_fill(const ErplDesignArgs a, double* __restrict__ out, int* flag) {
  __shared__ uint32_t keys[kDesignBlock * 6];
  const uint32_t row = blockIdx.y, g = a.first_row + row;
  const int64_t c0 = (int64_t)blockIdx.x * kDesignBlock;
  const int64_t c = c0 + threadIdx.x;
  uint32_t rho0 = 0;
  if (a.kind != ERPL_DESIGN_RANDOM) {
    const int64_t c1 = c0 + kDesignBlock - 1 < a.count - 1 ? c0 + kDesignBlock - 1 : a.count - 1;
    rho0 = (uint32_t)(a.first + c0) / a.m;
    const uint32_t n_rep = (uint32_t)(a.first + c1) / a.m - rho0 + 1u;   // <= 256: the workgroup has 256 columns
    if (threadIdx.x < n_rep) {
      const ErplDesignKeys K = erpl_design_keys(a.seed, g, rho0 + threadIdx.x);
#pragma unroll
      for (int j = 0; j < 6; ++j) keys[threadIdx.x * 6 + j] = K.k[j];
    }
    __syncthreads();
  }
  if (c >= a.count) return;
  const uint32_t i = (uint32_t)(a.first + c);
  uint32_t rho = 0, l = i;
  if (a.m != a.n) { rho = i / a.m; l = i - rho * a.m; }
  uint32_t k[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  if (a.kind != ERPL_DESIGN_RANDOM) {
#pragma unroll
    for (int j = 0; j < 6; ++j) k[j] = keys[(rho - rho0) * 6 + j];
  }
  const bool normal = (a.normal[row >> 5] >> (row & 31u)) & 1u;
  bool capped = false;
  const double v = erpl_design_value(a.seed, a.kind, normal, g, i, k, a.b, a.m, l, &capped);
  if (capped) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  out[(int64_t)row * a.ld + c] = v;
}

// the refusals of erpl_mc_design and erpl_mc_design_host, in the order of the header
int design_check(const erpl_design_spec* s, const uint8_t* kinds, int64_t first, int64_t count, const double* out, int64_t ld) {
  if (!s) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  if (!kinds) return erpl_fail(ERPL_ERR_INVALID, "kinds is NULL");
  if (!out) return erpl_fail(ERPL_ERR_INVALID, "out is NULL");
  if (s->kind != ERPL_DESIGN_RANDOM && s->kind != ERPL_DESIGN_LHS && s->kind != ERPL_DESIGN_LHS_CENTRED)
    return erpl_fail(ERPL_ERR_INVALID, "unknown kind %d", s->kind);
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
  return ERPL_OK;
}

int design_capped() { return erpl_fail(ERPL_ERR_INTERNAL, "erpl_mc_design: a cycle walk reached %d trips; its values are NaN", ERPL_DESIGN_WALK_CAP); }
}  // namespace

// erpl_mc_synchronize and erpl_mc_check_batch(ticket <= 0), behind their own waits: waits for the latest design call and
// reports a walk that was given up, once
__attribute__((visibility("hidden"))) int erpl_design_check_flag(erpl_ctx* c) {
  if (!c->design_flag) return ERPL_OK;
  HIP_TRY(hipEventSynchronize(c->design_ev));
  if (*(volatile int*)c->design_flag == 0) return ERPL_OK;
  *(volatile int*)c->design_flag = 0;
  return design_capped();
}

// the pinned flag word and the event of the context, made by the first call of erpl_mc_design or erpl_mc_qmc
__attribute__((visibility("hidden"))) int erpl_design_flag_init(erpl_ctx* c) {
  if (c->design_flag) return ERPL_OK;
  HIP_TRY(hipEventCreateWithFlags(&c->design_ev, hipEventDisableTiming));
  int* flag = nullptr;
  HIP_TRY(hipHostMalloc((void**)&flag, sizeof(int), hipHostMallocDefault));
  *flag = 0;
  c->design_flag = flag;
  return ERPL_OK;
}

extern "C" {

int erpl_mc_design_defaults(erpl_design_spec* spec) {
  if (!spec) return erpl_fail(ERPL_ERR_INVALID, "spec is NULL");
  *spec = erpl_design_spec{};
  spec->kind = ERPL_DESIGN_LHS;
  spec->rows = 1;
  spec->n = 1;
  return ERPL_OK;
}

int erpl_mc_design(erpl_ctx* c, const erpl_design_spec* spec, const uint8_t* kinds, int64_t first, int64_t count, double* out,
                   int64_t ld, void* stream) {
  ERPL_TRY(design_check(spec, kinds, first, count, out, ld));
  if (!c) return erpl_fail(ERPL_ERR_INVALID, "NULL ctx");
  if (count == 0) return ERPL_OK;
  HIP_TRY(hipSetDevice(c->device));
  ERPL_TRY(erpl_design_flag_init(c));
  ErplDesignArgs a = {};
  a.seed = spec->seed;
  a.first = first; a.count = count; a.ld = ld;
  a.n = (uint32_t)spec->n;
  a.m = (uint32_t)(spec->block ? spec->block : spec->n);
  a.b = erpl_design_half_bits(a.m);
  a.first_row = (uint32_t)spec->first_row;
  a.kind = spec->kind;
  for (int32_t r = 0; r < spec->rows; ++r)
    if (kinds[r] == ERPL_DESIGN_NORMAL) a.normal[r >> 5] |= 1u << (r & 31);
  const dim3 grid((unsigned)((count + kDesignBlock - 1) / kDesignBlock), (unsigned)spec->rows);
  hipLaunchKernelGGL(erpl_design_fill, grid, dim3(kDesignBlock), 0, (hipStream_t)stream, a, out, c->design_flag);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->design_ev, (hipStream_t)stream));
  return ERPL_OK;
}

int erpl_mc_design_host(const erpl_design_spec* spec, const uint8_t* kinds, int64_t first, int64_t count, double* out, int64_t ld) {
  ERPL_TRY(design_check(spec, kinds, first, count, out, ld));
  if (count == 0) return ERPL_OK;
  const uint64_t seed = spec->seed;
  const uint32_t m = (uint32_t)(spec->block ? spec->block : spec->n), b = erpl_design_half_bits(m);
  const int kind = spec->kind;
  const int nthr = host_threads(0, count);
  std::vector<char> capped(nthr, 0);
  run_threads(nthr, [&](int w) {
    const int64_t lo = count * w / nthr, hi = count * (w + 1) / nthr;
    for (int32_t r = 0; r < spec->rows; ++r) {
      const uint32_t g = (uint32_t)(spec->first_row + r);
      ErplDesignKeys K = {};
      int64_t have = -1;    // the replicate K belongs to
      for (int64_t c = lo; c < hi; ++c) {
        const uint32_t i = (uint32_t)(first + c), rho = i / m, l = i - rho * m;
        if (kind != ERPL_DESIGN_RANDOM && have != (int64_t)rho) { K = erpl_design_keys(seed, g, rho); have = rho; }
        bool cap = false;
        out[(int64_t)r * ld + c] = erpl_design_value(seed, kind, kinds[r] == ERPL_DESIGN_NORMAL, g, i, K.k, b, m, l, &cap);
        if (cap) capped[w] = 1;
      }
    }
  });
  for (char f : capped)
    if (f) return design_capped();
  return ERPL_OK;
}

}  // extern "C"
