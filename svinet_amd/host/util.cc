// util.cc -- see util.hh.
#include "util.hh"

#include <sched.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <thread>

#include "svils.h"

namespace svinet {

void throw_svils(const char *what, int rc) { throw SvilsError(rc, std::string(what) + " failed: " + svils_last_error()); }

FILE *open_or_die(const std::string &path, const char *what, const char *mode) {
  FILE *f = fopen(path.c_str(), mode);
  if (!f) {
    printf("cannot open %s file:%s\n", what, strerror(errno));
    exit(-1);
  }
  return f;
}

unsigned usable_cpus() {
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n ? n : 1u, (unsigned)CPU_COUNT(&set));
  double quota = 0.0;
  if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char a[64];
    long per = 0;
    if (fscanf(f, "%63s %ld", a, &per) == 2 && strcmp(a, "max") != 0 && per > 0) quota = atof(a) / (double)per;
    fclose(f);
  } else if (FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
    long q = -1, per = 100000;
    if (fscanf(g, "%ld", &q) != 1) q = -1;
    fclose(g);
    if (FILE *h2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h2, "%ld", &per) != 1) per = 100000; fclose(h2); }
    if (q > 0 && per > 0) quota = (double)q / (double)per;
  }
  if (quota >= 1.0) n = std::min<unsigned>(n, (unsigned)(quota + 0.5));
  return std::max(1u, n);
}

double now_s() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

}  // namespace svinet
