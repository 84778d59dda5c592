// Micro-benchmark: does the HIP runtime keep a pool of hardware queues per stream priority?  (a
// lane's sweep stream at four queues.)  On each of N streams one single-workgroup kernel spins for about 2 ms of the
// constant wall clock (bounded: the loop also ends after kMaxPolls polls).  Streams that share a hardware queue run their
// kernels one after the other, so the wall time from the first launch to the last completion counts the queues:
// 8 default-priority streams on four queues take twice what 4 take; 4 default + 4 of another priority take what 4 take
// if that priority has queues of its own.  Also prints, from the kernels' own clock stamps, how many ran at a time.
//   hipcc --offload-arch=gfx950 -O3 queue_pools.hip -o queue_pools && ./queue_pools
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <vector>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

constexpr int kMaxStreams = 8;
constexpr int kMaxPolls = 4000000;   // hard cap of the spin loop (a poll of the wall clock takes well over 10 ns)

__global__ __launch_bounds__(64) void spin(unsigned long long ticks, unsigned long long* stamp) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long t = t0;
  for (int i = 0; i < kMaxPolls && t - t0 < ticks; ++i) t = wall_clock64();
  if (threadIdx.x == 0) { stamp[0] = t0; stamp[1] = t; }
}

// n_default streams of the default priority and n_prio streams of priority `prio`; three timed repetitions
static void run_case(const char* name, int n_default, int n_prio, int prio, unsigned long long ticks, double tick_ms,
                     unsigned long long* d_stamp) {
  const int n = n_default + n_prio;
  if (n > kMaxStreams) { printf("%s: too many streams\n", name); exit(1); }
  hipStream_t st[kMaxStreams];
  for (int i = 0; i < n; ++i) {
    if (i < n_default) CHECK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    else CHECK(hipStreamCreateWithPriority(&st[i], hipStreamNonBlocking, prio));
  }
  // the runtime binds a stream to its hardware queue on first use: one untimed round
  for (int i = 0; i < n; ++i) hipLaunchKernelGGL(spin, dim3(1), dim3(64), 0, st[i], ticks / 16, d_stamp + 2 * i);
  for (int i = 0; i < n; ++i) CHECK(hipStreamSynchronize(st[i]));
  for (int rep = 0; rep < 3; ++rep) {
    const auto w0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(spin, dim3(1), dim3(64), 0, st[i], ticks, d_stamp + 2 * i);
    for (int i = 0; i < n; ++i) CHECK(hipStreamSynchronize(st[i]));
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    unsigned long long h[2 * kMaxStreams];
    CHECK(hipMemcpy(h, d_stamp, (size_t)(2 * n) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // kernels running at a time: sweep over the start (+1) and end (-1) stamps
    std::vector<std::pair<unsigned long long, int>> ev;
    unsigned long long lo = h[0], hi = h[1];
    for (int i = 0; i < n; ++i) {
      ev.push_back({h[2 * i], +1}); ev.push_back({h[2 * i + 1], -1});
      lo = std::min(lo, h[2 * i]); hi = std::max(hi, h[2 * i + 1]);
    }
    std::sort(ev.begin(), ev.end());
    int run = 0, peak = 0;
    for (auto& e : ev) { run += e.second; peak = std::max(peak, run); }
    printf("%-44s rep %d: wall %7.3f ms, device span %7.3f ms, at most %d kernels at a time\n", name, rep, wall_ms,
           (double)(hi - lo) * tick_ms, peak);
  }
  for (int i = 0; i < n; ++i) CHECK(hipStreamDestroy(st[i]));
}

int main() {
  int least = 0, greatest = 0, khz = 0;
  CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
  if (khz <= 0) khz = 100000;
  const char* q = getenv("GPU_MAX_HW_QUEUES");
  printf("GPU_MAX_HW_QUEUES=%s, stream priority range: least %d, greatest %d, wall clock %d kHz\n", q ? q : "(unset)", least,
         greatest, khz);
  const unsigned long long ticks = (unsigned long long)khz * 2ull;   // 2 ms
  const double tick_ms = 1.0 / (double)khz;
  unsigned long long* d_stamp;
  CHECK(hipMalloc(&d_stamp, 2 * kMaxStreams * sizeof(unsigned long long)));
  run_case("4 default", 4, 0, 0, ticks, tick_ms, d_stamp);
  run_case("8 default", 8, 0, 0, ticks, tick_ms, d_stamp);
  if (least == greatest) {
    printf("the priority range is degenerate: no second pool to ask for\n");
  } else {
    run_case("4 default + 4 greatest priority", 4, 4, greatest, ticks, tick_ms, d_stamp);
    run_case("4 default + 4 least priority", 4, 4, least, ticks, tick_ms, d_stamp);
  }
  CHECK(hipFree(d_stamp));
  return 0;
}
