// util.hh -- what the host drivers share: the error of a failed svils_* call, output files, usable CPUs, a clock.
#pragma once
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace svinet {

// a failed svils_* call of a tool driver (findk.cc, lcstats.cc); rc: its svils_error.  main.cc and capi.cc catch it.
struct SvilsError : std::runtime_error {
  SvilsError(int code, const std::string &msg) : std::runtime_error(msg), rc(code) {}
  int rc;
};

// throws SvilsError(rc, "<what> failed: <svils_last_error()>")
[[noreturn]] void throw_svils(const char *what, int rc);

// fopen(path, mode), or the reference's "cannot open <what> file:<strerror>" on stdout and exit(-1)
FILE *open_or_die(const std::string &path, const char *what, const char *mode = "w");

// CPUs this process may really use: the affinity mask and the cgroup CPU quota (v2 cpu.max, v1 cfs_quota_us), not the
// machine's core count -- a container with a 16-CPU quota on a 256-core host gains nothing from 64 threads
unsigned usable_cpus();

double now_s();   // CLOCK_MONOTONIC in seconds

// psi(x), x > 0, of the host loops: recurrence up to x >= 6, then the asymptotic series (double accurate)
inline double digamma(double x) {
  double r = 0;
  while (x < 6) { r -= 1 / x; x += 1; }
  const double f = 1 / (x * x);
  return r + std::log(x) - 0.5 / x -
         f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
}

}  // namespace svinet
