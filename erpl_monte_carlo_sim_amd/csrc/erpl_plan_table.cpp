// erpl_plan_table.cpp — prints what erpl_plan.h decides, for tests/test_plan.py (host compiler only, no HIP).
// stdin, one request per line:
//   depth <queues>
//   plan <submit> <queues> <depth> <in_flight> <precision> <n> <n_traj> <adopt> <sweep_pool> <chunk> <waves> <seen_mean_steps>
//        <two_priorities> <pool_on> <lane_stream: 0 none, 1 default priority, 2 pool> <n_cu> <max_time> <dt_flight>
// stdout, one line per request: the depth, or
//   <rotate> <waves_per_simd> <chunk_steps> <n_phases> <adopt_lanes> <sweep_waves> <tail: 0 main, 1 own, 2 pool> <w6> <w7> <pool_on>
#include <stdio.h>
#include <string.h>

#include "erpl_plan.h"

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    int queues = 0;
    if (sscanf(line, "depth %d", &queues) == 1) { printf("%d\n", erpl_default_depth(queues)); continue; }
    int submit, two, pool_on, lane_stream;
    long long n, n_traj;
    ErplPlanIn in;
    if (sscanf(line, "plan %d %d %d %d %d %lld %lld %d %d %d %d %lf %d %d %d %d %lf %lf", &submit, &in.queues, &in.depth,
               &in.in_flight, &in.precision, &n, &n_traj, &in.adopt, &in.sweep_pool, &in.chunk, &in.waves, &in.seen_mean_steps,
               &two, &pool_on, &lane_stream, &in.n_cu, &in.max_time, &in.dt_flight) != 18) {
      fprintf(stderr, "bad request: %s", line);
      return 1;
    }
    in.submit = submit != 0; in.n = n; in.n_traj = n_traj;
    // erpl_mc_submit_batch: ask for the lane's stream; a lane that has one already keeps the one it has
    bool latch = pool_on != 0;
    if (in.submit) in.sweep = erpl_sweep_stream(in, latch, [&] { return two != 0; });
    in.lane_stream_pool = lane_stream ? lane_stream == 2 : in.sweep == ERPL_SWEEP_POOL;
    const ErplPlan p = erpl_plan_batch(in);
    printf("%d %d %d %d %d %d %d %d %d %d\n", (int)p.rotate_sets, p.waves_per_simd, p.chunk_steps, p.n_phases, p.adopt_lanes,
           p.sweep_waves, p.tail_on_sweep ? (p.pool ? 2 : 1) : 0, p.adopt_lanes, erpl_plan_word7(p), (int)latch);
  }
  return 0;
}
