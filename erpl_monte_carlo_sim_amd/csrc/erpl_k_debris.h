// erpl_k_debris.h — kernels 8 to 10 (gate build only): where the fragments of every captured trajectory of a batch fall if
// the vehicle breaks up at a node (erpl_mc_debris).  A job is (trajectory j, node k, fragment f).  The prefix kernel marks the
// jobs whose node lies below the usable prefix.  The fall kernel runs one lane per job: the state of the node's record, its
// velocity changed by the fragment's break-up impulse (erpl_debris.h), falls under gravity, the drag of a constant ballistic
// coefficient and the sample's own wind - the gate's device functions, no contraction - by classic RK4 whose step the rule
// of erpl_debris.h halves where drag is stiff, until it crosses the ground plane.  The summary kernel reduces a
// trajectory's jobs under the total order of erpl_k_envelope.h, one wave per trajectory.  No kernel has atomics or
// cross-lane arithmetic in a value: the bytes of a column depend on the trajectory's own records, its sample's wind and the
// spec alone, whatever else shares its wave, workgroup or launch.
//
// Every loop is bounded: the fall by max_steps RK4 steps of any size (and it leaves at the first non-finite entry), the
// step rule by ERPL_DEBRIS_MAX_HALVINGS, the direction by ERPL_DEBRIS_MAX_TRIES, the prefix scan by the records a node can sit
// on, the table searches as in erpl_k_lookup.h.
namespace {

constexpr int kDebrisBlock = 64;   // one wave per workgroup, as the impact points: a slot frees when its slowest lane lands

// The envelope's total order, the impact points' wave fold, finiteness test and crossing rule, RESTATED: the same expressions in
// functions of this file's own.  A second caller of env_better, env_take, iip_wave_best or iip_inside changes the code of the
// envelope and the impact-point summary kernels (DESIGN.md 8.11 met the same with env_reduce), and those must not move.
template <bool MAX>
__device__ __forceinline__ EnvBest debris_better(EnvBest x, EnvBest o) {
  // (selects on the two fields, not on the structs: a choice between two structs by reference became an indexed stack
  // object in the summary kernel, 40 bytes of scratch)
  const bool o_wins = MAX ? (o.v > x.v) : (o.v < x.v);
  const bool x_wins = MAX ? (x.v > o.v) : (x.v < o.v);
  const bool take = o.i != kEnvNone && (x.i == kEnvNone || o_wins || (!x_wins && o.i < x.i));
  EnvBest r;
  r.v = take ? o.v : x.v; r.i = take ? o.i : x.i;
  return r;
}
template <bool MAX>
__device__ __forceinline__ void debris_take(EnvBest& x, double v, long long r) {
  const bool wins = MAX ? (v > x.v) : (v < x.v);
  const bool loses = MAX ? (x.v > v) : (x.v < v);
  const bool take = __builtin_isfinite(v) && (x.i == kEnvNone || wins || (!loses && r < x.i));
  x.v = take ? v : x.v; x.i = take ? r : x.i;
}
__device__ __forceinline__ EnvBest debris_none() {
  EnvBest x;
  x.v = 0.0; x.i = kEnvNone;
  return x;
}
template <bool MAX>
__device__ __forceinline__ EnvBest debris_wave_best(EnvBest x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    EnvBest o;
    o.v = __shfl_down(x.v, off);
    o.i = __shfl_down(x.i, off);
    x = debris_better<MAX>(x, o);   // (a lane whose partner is past the wave reads itself)
  }
  EnvBest r;
  r.v = __shfl(x.v, 0);
  r.i = __shfl(x.i, 0);
  return r;
}
__device__ __forceinline__ bool debris_finite6(const real (&s)[6]) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) ok = ok && __builtin_isfinite(s[c]);
  return ok;
}
__device__ __forceinline__ bool debris_inside(const double* vx, const double* vy, int nv, double x, double y) {
  bool in = false;
  for (int i = 0, jv = nv - 1; i < nv; jv = i++)
    if ((vy[i] > y) != (vy[jv] > y) && x < (vx[jv] - vx[i]) * (y - vy[i]) / (vy[jv] - vy[i]) + vx[i]) in = !in;
  return in;
}

// d/dt of (x, y, z, vx, vy, vz) for a fragment of ballistic coefficient beta; returns the drag rate k (1/s)
__device__ __forceinline__ real debris_rhs(const Shared& C, int64_t id, WindCache& wc, real beta, const real (&s)[6],
                                           real (&ds)[6]) {
  const ErplScalars<real>& S = *C.S;
  real T, P;
  atmosphere(S, s[2], T, P);
  const real rho = m_div(P, S.Rg * T);
  const real g = gravity_at(S, s[2]);
  real w[3];
  wind_at(C, id, s[2], wc, w);
  const real vr0 = s[3] - w[0], vr1 = s[4] - w[1], vr2 = s[5] - w[2];
  const real vn = m_sqrt((vr0 * vr0 + vr1 * vr1) + vr2 * vr2);
  const real k = m_div(((real)0.5 * rho) * vn, beta);
  ds[0] = s[3]; ds[1] = s[4]; ds[2] = s[5];
  ds[3] = -k * vr0; ds[4] = -k * vr1; ds[5] = -k * vr2 - g;
  return k;
}

// The number of evaluated nodes of trajectory j (the rule of iip_evaluated_nodes, restated over this call's own arguments:
// the nodes k with k * record_stride < u, u the usable prefix), by the 64 lanes of one wave.
__device__ __forceinline__ int64_t debris_evaluated_nodes(const ErplKArgs& a, const ErplDebrisArgs& q, int64_t j) {
  int64_t len = a.traj_len[j];
  len = (len < 0) ? 0 : ((len > a.traj_cap) ? a.traj_cap : len);   // never past the trajectory's own slots
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;
  const int64_t stride = q.record_stride;
  int64_t scan = (int64_t)(q.n_nodes - 1) * stride + 1;
  scan = (scan < len) ? scan : len;
  EnvBest mine = debris_none();
  for (int64_t r = threadIdx.x; r < scan; r += kDebrisBlock) {
    const double* rec = recs + r * ERPL_TRAJ_DIM;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < ERPL_TRAJ_DIM; ++c) ok = ok && __builtin_isfinite(rec[c]);
    if (!ok) { mine.i = r; break; }
  }
  const EnvBest first_bad = debris_wave_best<false>(mine);
  const int64_t u = (first_bad.i == kEnvNone) ? scan : first_bad.i;
  const int64_t nodes = (u + stride - 1) / stride;
  return (nodes < q.n_nodes) ? nodes : q.n_nodes;
}

// The prefix kernel, ahead of the fall: grid = n_traj workgroups of one wave; the X slot of every job of trajectory j becomes
// 1.0 if its node is evaluated and NaN if not, and the number of evaluated nodes goes to the NODES row of the summary.
__global__ __launch_bounds__(kDebrisBlock) void erpl_debris_prefix_f64(const ErplKArgs a, const ErplDebrisArgs q) {
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  const int64_t nodes = debris_evaluated_nodes(a, q, j);
  const int64_t rows = (int64_t)q.n_nodes * q.n_fragments, live = nodes * q.n_fragments;
  for (int64_t i = threadIdx.x; i < rows; i += kDebrisBlock)
    q.values[((int64_t)ERPL_IIP_CH_X * rows + i) * q.ld + q.col0 + j] = (i < live) ? 1.0 : (double)NAN;
  if (q.summary && threadIdx.x == 0) q.summary[(int64_t)ERPL_DEBRIS_NODES * a.n_traj + j] = (double)nodes;
}

// The fall: grid (ceil(n_traj / 64), n_nodes * n_fragments), a wave holds 64 neighbouring trajectories at one (k, f).
// blockIdx.y is a dispatch slot: slot y runs fragment fr.order[y / n_nodes] at node n_nodes - 1 - y % n_nodes, so the
// fragments of the smallest beta (the longest falls) are dispatched first and, within a fragment, the latest node first
// (what the dispatch order is worth).  A lane's step differs from its neighbour's, but every lane takes one RK4
// step per trip: the step rule adds no divergence beyond the differing step counts.
__global__ __launch_bounds__(kDebrisBlock) void erpl_debris_fall_f64(const ErplKArgs a, const ErplScalars<real> S,
                                                                      const ErplDebrisArgs q, const ErplDebrisFragments fr) {
  __shared__ LdsTables L;
  extern __shared__ real debris_alt[];   // the wind altitude grid: max(k_wind, 1) values
  stage_tables(L, debris_alt, a.tables, a.alt_grid, a.k_wind);   // (ends in a barrier)
  const int64_t j = (int64_t)blockIdx.x * kDebrisBlock + threadIdx.x;
  const int64_t rows = (int64_t)q.n_nodes * q.n_fragments;
  if (j >= a.n_traj || (int64_t)blockIdx.y >= rows) return;
  const int slot = (int)blockIdx.y / q.n_nodes;
  const int f = fr.order[slot];
  const int64_t k = (int64_t)(q.n_nodes - 1) - (int64_t)((int)blockIdx.y - slot * q.n_nodes);
  const int64_t row = k * q.n_fragments + f;
  double out[ERPL_IIP_CH_COUNT];
#pragma unroll
  for (int c = 0; c < ERPL_IIP_CH_COUNT; ++c) out[c] = (double)NAN;
  // evaluated iff the prefix kernel left 1.0 in the job's own X slot (no other lane reads or writes that slot)
  const bool evaluated = q.values[((int64_t)ERPL_IIP_CH_X * rows + row) * q.ld + q.col0 + j] == 1.0;
  if (evaluated) {
    const double* rec = a.traj + (j * a.traj_cap + k * (int64_t)q.record_stride) * ERPL_TRAJ_DIM;
    const int64_t id = a.traj_ids[j];
    const real beta = fr.beta[f], dv = fr.dv[f];
    real s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = rec[1 + c];
    if (dv != (real)0) {   // (no draw for a fragment without an impulse: the velocity keeps the record's bits)
      double d[3];
      erpl_debris_direction(q.seed, (uint64_t)id, (uint32_t)k, (uint32_t)f, d);
#pragma unroll
      for (int c = 0; c < 3; ++c) s[3 + c] = s[3 + c] + dv * d[c];
    }
    const real speed = m_sqrt((s[3] * s[3] + s[4] * s[4]) + s[5] * s[5]);
    if (speed <= (real)1e6 && s[2] >= (real)-1e5) {   // of physical size, after the impulse
      bool landed = false;
      if (s[2] <= q.ground) {
        out[ERPL_IIP_CH_X] = s[0]; out[ERPL_IIP_CH_Y] = s[1];
        out[ERPL_IIP_CH_TFALL] = 0.0; out[ERPL_IIP_CH_VIMPACT] = speed;
        landed = true;
      } else {
        Shared C;
        C.S = &S; C.L = &L; C.alt = debris_alt; C.has_wind = a.k_wind > 0; C.motor_kind = a.motor_kind;
        WindCache wc;
        wc.lo = 1; wc.hi = 0; wc.x0 = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) { wc.y0[c] = 0; wc.s[c] = 0; }
        const real dt = q.dt, dt2 = (real)0.5 * q.dt, dt6 = q.dt / (real)6.0;
        int64_t ticks = 0;
        for (int n = 0; n < q.max_steps; ++n) {
          real k1[6], k2[6], k3[6], k4[6], y[6], sn[6];
          const real k0 = debris_rhs(C, id, wc, beta, s, k1);
          real scale;
          const int m = erpl_debris_halvings(k0, dt, q.stiff_limit, &scale);
          const real h = dt * scale, h2 = dt2 * scale, h6 = dt6 * scale;
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + h2 * k1[c];
          (void)debris_rhs(C, id, wc, beta, y, k2);
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + h2 * k2[c];
          (void)debris_rhs(C, id, wc, beta, y, k3);
#pragma unroll
          for (int c = 0; c < 6; ++c) y[c] = s[c] + h * k3[c];
          (void)debris_rhs(C, id, wc, beta, y, k4);
#pragma unroll
          for (int c = 0; c < 6; ++c) sn[c] = s[c] + h6 * ((k1[c] + (real)2.0 * k2[c]) + ((real)2.0 * k3[c] + k4[c]));
          if (!debris_finite6(sn)) break;   // does not land
          if (sn[2] <= q.ground) {
            const real wq = (s[2] - q.ground) / (s[2] - sn[2]);
            out[ERPL_IIP_CH_X] = s[0] + (sn[0] - s[0]) * wq;
            out[ERPL_IIP_CH_Y] = s[1] + (sn[1] - s[1]) * wq;
            out[ERPL_IIP_CH_TFALL] = erpl_debris_tfall(ticks, wq, m, dt);
            const real v0 = s[3] + (sn[3] - s[3]) * wq, v1 = s[4] + (sn[4] - s[4]) * wq, v2 = s[5] + (sn[5] - s[5]) * wq;
            out[ERPL_IIP_CH_VIMPACT] = m_sqrt((v0 * v0 + v1 * v1) + v2 * v2);
            landed = true;
            break;
          }
          ticks += erpl_debris_step_ticks(m);
#pragma unroll
          for (int c = 0; c < 6; ++c) s[c] = sn[c];
        }
      }
      if (landed) {
        const real dx = out[ERPL_IIP_CH_X] - q.origin_x, dy = out[ERPL_IIP_CH_Y] - q.origin_y;
        out[ERPL_IIP_CH_RANGE] = m_sqrt(dx * dx + dy * dy);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < ERPL_IIP_CH_COUNT; ++c) q.values[((int64_t)c * rows + row) * q.ld + q.col0 + j] = out[c];
}

// The summary [ERPL_DEBRIS_DIM][n_traj] of the values the fall kernel left: grid = n_traj workgroups of one wave, lane t takes
// the nodes t, t + 64, ... and walks a node's fragments in index order.  (value, job index k * n_fragments + f) pairs under
// the envelope's order, folded as the impact points fold them: ties go to the lowest index, that is the earliest node and there the lowest fragment.
__global__ __launch_bounds__(kDebrisBlock) void erpl_debris_summary_f64(const ErplKArgs a, const ErplDebrisArgs q,
                                                                         const ErplIipKeepIn keep) {
  __shared__ double s_vx[ERPL_IIP_MAX_VERTICES], s_vy[ERPL_IIP_MAX_VERTICES];
  const int tid = threadIdx.x;
  const int nv = keep.n;
  if (tid < nv) { s_vx[tid] = keep.x[tid]; s_vy[tid] = keep.y[tid]; }
  __syncthreads();
  const int64_t j = blockIdx.x;
  if (j >= a.n_traj) return;
  const double* __restrict__ recs = a.traj + j * a.traj_cap * ERPL_TRAJ_DIM;
  const int64_t stride = q.record_stride, F = q.n_fragments;
  const int64_t rows = (int64_t)q.n_nodes * F;
  int64_t nodes = (int64_t)q.summary[(int64_t)ERPL_DEBRIS_NODES * a.n_traj + j];   // the prefix kernel's count
  nodes = (nodes < 0) ? 0 : ((nodes > q.n_nodes) ? q.n_nodes : nodes);
  const double* X = q.values + ((int64_t)ERPL_IIP_CH_X * rows) * q.ld + q.col0 + j;
  const double* Y = q.values + ((int64_t)ERPL_IIP_CH_Y * rows) * q.ld + q.col0 + j;
  const double* R = q.values + ((int64_t)ERPL_IIP_CH_RANGE * rows) * q.ld + q.col0 + j;
  const double* TF = q.values + ((int64_t)ERPL_IIP_CH_TFALL * rows) * q.ld + q.col0 + j;
  double row[ERPL_DEBRIS_DIM];
#pragma unroll
  for (int c = 0; c < ERPL_DEBRIS_DIM; ++c) row[c] = (double)NAN;
  int landed = 0, outside = 0;
  if (nodes > 0) {   // (uniform over the wave)
    const double t0 = recs[0];
    EnvBest far = debris_none(), slow = debris_none(), wide = debris_none(), ex = debris_none();
    for (int64_t k = tid; k < nodes; k += kDebrisBlock) {
      double xlo = 0.0, xhi = 0.0, ylo = 0.0, yhi = 0.0;
      bool any = false;
      for (int64_t f = 0; f < F; ++f) {
        const int64_t i = k * F + f;
        const double x = X[i * q.ld], y = Y[i * q.ld];
        if (!__builtin_isfinite(x)) continue;   // a landed job: all five channels are finite
        ++landed;
        debris_take<true>(far, R[i * q.ld], i);
        debris_take<true>(slow, TF[i * q.ld], i);
        if (nv > 0 && !debris_inside(s_vx, s_vy, nv, x, y)) {
          ++outside;
          if (ex.i == kEnvNone) ex.i = i;   // (a lane meets its jobs in ascending index order)
        }
        if (!any) { xlo = xhi = x; ylo = yhi = y; any = true; }
        else {
          xlo = (x < xlo) ? x : xlo; xhi = (x > xhi) ? x : xhi;
          ylo = (y < ylo) ? y : ylo; yhi = (y > yhi) ? y : yhi;
        }
      }
      if (any) {
        const double dx = xhi - xlo, dy = yhi - ylo;
        debris_take<true>(wide, sqrt(dx * dx + dy * dy), k);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {   // integer sums: their order changes nothing
      landed += __shfl_down(landed, off);
      outside += __shfl_down(outside, off);
    }
    const EnvBest bfar = debris_wave_best<true>(far), bslow = debris_wave_best<true>(slow), bwide = debris_wave_best<true>(wide);
    const EnvBest bex = debris_wave_best<false>(ex);
    if (tid == 0) {
      if (bfar.i != kEnvNone) {
        const int64_t kf = bfar.i / F;
        row[ERPL_DEBRIS_MAX_RANGE] = bfar.v; row[ERPL_DEBRIS_MAX_RANGE_TIME] = recs[kf * stride * ERPL_TRAJ_DIM] - t0;
        row[ERPL_DEBRIS_MAX_RANGE_X] = X[bfar.i * q.ld]; row[ERPL_DEBRIS_MAX_RANGE_Y] = Y[bfar.i * q.ld];
        row[ERPL_DEBRIS_MAX_RANGE_FRAGMENT] = (double)(bfar.i - kf * F);
      }
      if (bex.i != kEnvNone) {
        const int64_t ke = bex.i / F;
        row[ERPL_DEBRIS_EXIT_TIME] = recs[ke * stride * ERPL_TRAJ_DIM] - t0;
        row[ERPL_DEBRIS_EXIT_FRAGMENT] = (double)(bex.i - ke * F);
        row[ERPL_DEBRIS_EXIT_X] = X[bex.i * q.ld]; row[ERPL_DEBRIS_EXIT_Y] = Y[bex.i * q.ld];
      }
      if (bslow.i != kEnvNone) {
        row[ERPL_DEBRIS_MAX_TFALL] = bslow.v;
        row[ERPL_DEBRIS_MAX_TFALL_TIME] = recs[(bslow.i / F) * stride * ERPL_TRAJ_DIM] - t0;
      }
      if (bwide.i != kEnvNone) {
        row[ERPL_DEBRIS_MAX_SPREAD] = bwide.v; row[ERPL_DEBRIS_MAX_SPREAD_TIME] = recs[bwide.i * stride * ERPL_TRAJ_DIM] - t0;
      }
    }
  }
  if (tid == 0) {
    if (nv > 0) row[ERPL_DEBRIS_OUTSIDE] = (double)outside;
    row[ERPL_DEBRIS_LANDED] = (double)landed; row[ERPL_DEBRIS_NODES] = (double)nodes;
#pragma unroll
    for (int c = 0; c < ERPL_DEBRIS_DIM; ++c) q.summary[(int64_t)c * a.n_traj + j] = row[c];
  }
}

}  // namespace
