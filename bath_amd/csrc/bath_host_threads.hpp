// bath_host_threads.hpp -- how many host threads a stage may start, and run_striped, which starts them over the independent items of
// a stage (the domain stages' ensembles, bath_domaindef.hip and bath_std_domains.hip; the profile builds of a calibration batch,
// bath_calibrate.hip).
// Thread count: the CPUs this process may run on (its affinity mask, not the machine's thread count: a GPU box hands a job a
// slice of its cores), at most 64, divided by the ranks that share the node -- LOCAL_WORLD_SIZE, which torch.distributed.run
// exports: one process per GPU, each with its own ensembles; BATH_HIP_HOST_THREADS overrides.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sched.h>
#include <thread>
#include <vector>

namespace bath {

// The cores a cgroup CPU quota leaves this process (cpu.max of cgroup v2, cpu.cfs_quota_us / cpu.cfs_period_us of v1), 0: no quota.
// A GPU box hands a job all 256 CPUs in its affinity mask and a quota of 16 cores: 64 threads that poll for their region's matrix
// then use the quota up within a scheduler period and the WHOLE process is throttled for the rest of it -- one --fs pass in four
// or five ran 10-15 ms long until round 4 found that in /sys/fs/cgroup/cpu.stat (nr_throttled).
inline int cgroup_quota_cores() {
  auto read2 = [](const char *path, long long *a, long long *b) -> bool {
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char x[64] = {0}, y[64] = {0};
    const int n = std::fscanf(f, "%63s %63s", x, y);
    std::fclose(f);
    if (n < 1 || std::strcmp(x, "max") == 0) return false;
    *a = std::atoll(x); *b = n >= 2 ? std::atoll(y) : 0;
    return true;
  };
  long long q = 0, per = 0;
  if (read2("/sys/fs/cgroup/cpu.max", &q, &per) && q > 0 && per > 0) return (int)std::max<long long>(1, (q + per - 1) / per);
  long long q1 = 0, p1 = 0, dummy = 0;
  if (read2("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", &q1, &dummy) && q1 > 0 && read2("/sys/fs/cgroup/cpu/cpu.cfs_period_us", &p1, &dummy) && p1 > 0)
    return (int)std::max<long long>(1, (q1 + p1 - 1) / p1);
  return 0;
}
inline int host_thread_count() {
  const char *e = std::getenv("BATH_HIP_HOST_THREADS");
  if (e && std::atoi(e) > 0) return std::atoi(e);
  static const int cached = [] {
    int usable = 0;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) usable = CPU_COUNT(&set);
    if (usable <= 0) usable = (int)std::max(1u, std::thread::hardware_concurrency());
    const int quota = cgroup_quota_cores();
    // (four times the quota: the threads sleep while they wait for their region's matrix, and 150 core-ms of tracebacks per pass are far
    // from a 16-core quota once nothing spins; 8 / 12 threads leave the ensembles on the pass's critical path: 74 / 69 ms per pass
    // against 64-65 with 16-64, and in the fast mode, where the ensembles ARE the critical path, 32 threads cost 3 ms against 64)
    if (quota > 0) usable = std::min(usable, std::max(2, quota * 4));
    int ranks = 1;
    if (const char *lw = std::getenv("LOCAL_WORLD_SIZE")) ranks = std::max(1, std::atoi(lw));
    return std::min(64, std::max(1, usable / ranks));
  }();
  return cached;
}

// Host threads for n items that are independent of each other (the regions of one block).  work(first, step) handles items first,
// first + step, ...; the threads draw single items from a shared counter, heaviest first (<weight>), so that they finish together.
template <class F, class W>
void run_striped(int64_t n, F &&work, W &&weight) {
  const int T = (int)std::min<int64_t>(n, host_thread_count());
  if (T <= 1) { work(0, 1); return; }
  std::vector<int64_t> order((size_t)n);
  for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return weight(a) > weight(b); });
  std::atomic<int64_t> next{0};
  std::vector<std::thread> th;
  for (int k = 0; k < T; k++)
    th.emplace_back([&] { for (int64_t j = next.fetch_add(1); j < n; j = next.fetch_add(1)) work(order[(size_t)j], n); });
  for (std::thread &t : th) t.join();
}

}  // namespace bath
