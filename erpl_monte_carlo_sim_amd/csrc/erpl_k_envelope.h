// erpl_k_envelope.h — kernel 4 (gate build only): the flight envelope of every captured trajectory of a batch
// (erpl_mc_flight_envelope).  One workgroup of kEnvBlock threads per trajectory; thread t takes the records t,
// t + kEnvBlock, ...  Three passes over the trajectory's records, each closed by workgroup reductions:
//   1. the usable prefix u: the first record with a non-finite entry (all 15 columns)
//   2. the apogee record a (first largest altitude below u) and the burnout record b (first ts > burn_time below u)
//   3. the maxima: angular rate and quaternion norm over r < u, everything that needs record_eval over r <= a,
//      and record b
// Every reduction folds (value, record index) pairs under a total order - better value, then lower index - so its result
// does not depend on the shape of the fold: no atomics, and the bytes of a trajectory's column depend on its own records
// and its sample's parameters alone.
namespace {

constexpr int kEnvBlock = 256;
constexpr int kEnvWaves = kEnvBlock / 64;
constexpr long long kEnvNone = 0x7fffffffffffffffLL;   // the index of "no record"

struct EnvBest {
  double v;
  long long i;
};
// the better of two candidates: MAX ? the larger value : the smaller; equal values (-0.0 and +0.0 too): the lower index
template <bool MAX>
__device__ __forceinline__ EnvBest env_better(const EnvBest& x, const EnvBest& o) {
  if (o.i == kEnvNone) return x;
  if (x.i == kEnvNone) return o;
  const bool o_wins = MAX ? (o.v > x.v) : (o.v < x.v);
  const bool x_wins = MAX ? (x.v > o.v) : (x.v < o.v);
  return (o_wins || (!x_wins && o.i < x.i)) ? o : x;
}
// a finite value of record r enters the running candidate of its thread
template <bool MAX>
__device__ __forceinline__ void env_take(EnvBest& x, double v, long long r) {
  if (!__builtin_isfinite(v)) return;
  EnvBest o;
  o.v = v; o.i = r;
  x = env_better<MAX>(x, o);
}
// the workgroup's best, returned to every thread; red: kEnvWaves entries of LDS, free again on return
template <bool MAX>
__device__ __forceinline__ EnvBest env_reduce(EnvBest x, EnvBest* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    EnvBest o;
    o.v = __shfl_down(x.v, off);
    o.i = __shfl_down(x.i, off);
    x = env_better<MAX>(x, o);   // (a lane whose partner is past the wave reads itself)
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  EnvBest r = red[0];
#pragma unroll
  for (int w = 1; w < kEnvWaves; ++w) r = env_better<MAX>(r, red[w]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ EnvBest env_none() {
  EnvBest x;
  x.v = 0.0; x.i = kEnvNone;
  return x;
}

// a.n_traj trajectories, a.traj_ids / a.traj / a.traj_cap / a.traj_len as erpl_out has them, a.summary = the envelope
// [ERPL_ENV_DIM][n_traj]; grid = n_traj workgroups of kEnvBlock threads.
__global__ __launch_bounds__(kEnvBlock) void erpl_envelope_f64(const ErplKArgs a, const ErplScalars<real> S) {
  __shared__ LdsTables L;
  __shared__ real alt_s[ERPL_MAX_WIND_KNOTS];
  __shared__ EnvBest red[kEnvWaves];
  __shared__ double row[ERPL_ENV_DIM];
  const int tid = threadIdx.x;
  if (tid < ERPL_ENV_DIM) row[tid] = (double)NAN;
  stage_tables(L, alt_s, a.tables, a.alt_grid, a.k_wind);   // (ends in a barrier)
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  Shared C;
  C.S = &S; C.L = &L; C.alt = alt_s; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
  const int64_t id = a.traj_ids[j];
  int64_t len = a.traj_len[j];
  len = (len < 0) ? 0 : ((len > a.traj_cap) ? a.traj_cap : len);   // never past the trajectory's own slots
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;

  // pass 1: the usable prefix
  EnvBest mine = env_none();
  for (int64_t r = tid; r < len; r += kEnvBlock) {
    const double* rec = recs + r * ERPL_TRAJ_DIM;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < ERPL_TRAJ_DIM; ++c) ok = ok && __builtin_isfinite(rec[c]);
    if (!ok) { mine.i = r; break; }
  }
  const EnvBest first_bad = env_reduce<false>(mine, red);
  const int64_t u = (first_bad.i == kEnvNone) ? len : first_bad.i;
  if (u > 0) {   // (uniform over the workgroup)
    LaneParams p;
    lane_params_of(a, S, id, p);
    const double t0 = recs[0];
    // pass 2: apogee and burnout records
    EnvBest top = env_none(), out = env_none();
    for (int64_t r = tid; r < u; r += kEnvBlock) {
      const double* rec = recs + r * ERPL_TRAJ_DIM;
      env_take<true>(top, rec[3], r);
      if (out.i == kEnvNone && rec[0] - t0 > p.burn) out.i = r;
    }
    const int64_t ap = env_reduce<true>(top, red).i;
    const int64_t bo = env_reduce<false>(out, red).i;
    // pass 3
    EnvBest q = env_none(), mach = env_none(), qa = env_none(), acc = env_none(), stab = env_none();
    EnvBest omega = env_none(), quat = env_none();
    double q_ts = 0.0, q_z = 0.0, q_mach = 0.0;   // of this thread's own max-q record
    for (int64_t r = tid; r < u; r += kEnvBlock) {
      const double* rec = recs + r * ERPL_TRAJ_DIM;
      {
        const double w = rec[7], x = rec[8], yy = rec[9], z = rec[10];
        env_take<true>(omega, fmax(fmax(fabs(rec[11]), fabs(rec[12])), fabs(rec[13])), r);
        env_take<true>(quat, fabs(sqrt(((w * w + x * x) + yy * yy) + z * z) - 1.0), r);
      }
      if (r > ap && r != bo) continue;
      const double ts = rec[0] - t0;
      real y[14];
#pragma unroll
      for (int c = 0; c < 14; ++c) y[c] = (real)rec[1 + c];
      RecordEval e;
      record_eval(C, p, id, ts, y, e);
      if (r <= ap) {
        const long long before = q.i;
        env_take<true>(q, e.qdyn, r);
        if (q.i != before) { q_ts = ts; q_z = y[2]; q_mach = e.mach; }
        env_take<true>(mach, e.mach, r);
        env_take<true>(qa, e.qdyn * m_atan2(m_sqrt(e.vb1 * e.vb1 + e.vb2 * e.vb2), e.vb0), r);
        env_take<true>(acc, (e.thrust - e.drag) / e.mass, r);
        env_take<false>(stab, e.margin, r);
      }
      if (r == bo) {   // one thread of the workgroup
        row[ERPL_ENV_BURNOUT_TIME] = ts;
        row[ERPL_ENV_BURNOUT_ALT] = y[2];
        row[ERPL_ENV_BURNOUT_SPEED] = m_sqrt((y[3] * y[3] + y[4] * y[4]) + y[5] * y[5]);
        row[ERPL_ENV_BURNOUT_STABILITY] = e.margin;
      }
    }
    const EnvBest bq = env_reduce<true>(q, red);
    const EnvBest bmach = env_reduce<true>(mach, red), bqa = env_reduce<true>(qa, red), bacc = env_reduce<true>(acc, red);
    const EnvBest bstab = env_reduce<false>(stab, red);
    const EnvBest bomega = env_reduce<true>(omega, red), bquat = env_reduce<true>(quat, red);
    if (bq.i != kEnvNone && q.i == bq.i) {   // the one thread whose own best is the workgroup's
      row[ERPL_ENV_MAX_Q] = bq.v;
      row[ERPL_ENV_MAX_Q_TIME] = q_ts; row[ERPL_ENV_MAX_Q_ALT] = q_z; row[ERPL_ENV_MAX_Q_MACH] = q_mach;
    }
    if (tid == 0) {
      if (bmach.i != kEnvNone) row[ERPL_ENV_MAX_MACH] = bmach.v;
      if (bqa.i != kEnvNone) row[ERPL_ENV_MAX_Q_ALPHA] = bqa.v;
      if (bacc.i != kEnvNone) row[ERPL_ENV_MAX_AXIAL_ACCEL] = bacc.v;
      if (bstab.i != kEnvNone) row[ERPL_ENV_MIN_STABILITY] = bstab.v;
      if (bomega.i != kEnvNone) row[ERPL_ENV_MAX_OMEGA] = bomega.v;
      if (bquat.i != kEnvNone) row[ERPL_ENV_MAX_QUAT_DEV] = bquat.v;
      row[ERPL_ENV_APOGEE_RECORD] = (double)ap;
    }
  }
  if (tid == 0) row[ERPL_ENV_USABLE] = (double)u;
  __syncthreads();
  if (tid < ERPL_ENV_DIM) a.summary[(int64_t)tid * a.n_traj + j] = row[tid];
}

}  // namespace
