// ppc.hh -- host side of `-ppc` and `-gen`: posterior predictive checks of a fitted model, and a network drawn from the
// model's prior.
//
// Same seam as the reference (src/mmsbgen.hh, used at src/main.cc:268-303):
//     MMSBGen mmsbgen(env, network, true);  mmsbgen.ppc();     /     MMSBGen mmsbgen(env, network, false);  mmsbgen.gen(alpha);
// The parameters of a replicate are drawn here (O(n K): draw_all, src/mmsbgen.cc:730-742, or estimate_all with -ppc-mean),
// every network is drawn and every statistic computed on the device through the svils_ppc_* entry points of
// include/svils.h, and the files are written here.  The random stream is this project's own, not
// GSL's: Philox4x32-10 keyed by (seed, replicate); stream 0 is the device's pair draw, streams 1 and 2 the Gamma variates
// of pi and beta.
#pragma once
#include <cstdint>
#include <string>

#include "env.hh"
#include "network.hh"

namespace svinet {

constexpr uint32_t kPpcStreamPi = 1, kPpcStreamBeta = 2;

// Philox4x32-10 (Salmon et al., SC'11): ctr [4], key [2] -> out [4]
void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
// Gamma(shape, 1), Marsaglia-Tsang, for variate (a, b) of `stream` under key (seed, r).  Attempt t reads block 2 t (the
// normal z = sqrt(-2 log(1 - u1)) cos(2 pi u2)) and block 2 t + 1 (accepted when log(1 - u3) < z^2 / 2 + d - d v + d log v);
// a shape below 1 is drawn at shape + 1 and scaled by (1 - ub)^(1 / shape), ub the first uniform of block 0xffffffff
double gamma_variate(double shape, uint32_t seed, uint32_t r, uint32_t a, uint32_t b, uint32_t stream);
// pi_i ~ Dirichlet(gam_i) [n][k]: variate (i, j) of stream 1, the row divided by its sum in ascending j (1 / k where it is 0)
void dirichlet_rows(const double *gam, uint32_t n, uint32_t k, uint32_t seed, uint32_t r, double *pi);
// beta_j ~ Beta(lam_j0, lam_j1) = g0 / (g0 + g1): variates (j, 0) and (j, 1) of stream 2
void beta_draws(const double *lam, uint32_t k, uint32_t seed, uint32_t r, double *beta);

struct PpcOptions {
  uint32_t draws = 100;   // -ppc-draws (ppc_ndraws, src/env.hh:452)
  uint32_t seed = 0;      // -seed
  uint32_t save = 0;      // -ppc-save <m>: ppc/<r>/network.dat of the first m replicates
  bool mean = false;      // -ppc-mean: every replicate from pi = gamma / sum, beta = l0 / (l0 + l1)
  bool orig = false;      // -ppc-orig: the K x K blockmodel, gamma.txt and beta.txt; block_size.txt / block_logpe.txt for the lc_* files
  bool hops = false;      // -ppc-hops: obs-hop.txt, ppc/ppc-hop.txt, ppc/obs-hops.txt, ppc/rep-hops.txt, ppc/hops-summary.txt
};

// beta.txt of an -orig fit (MMSBInferOrig::save_model): exactly k lines of exactly k rates in [0, 1] -> B [k][k].  0, or -1
// with a message on stderr that names the file and the line
int read_block_rates(const std::string &path, uint32_t k, double *B);
// -ppc in the output directory of a fit: gamma.txt / lambda.txt, files under ppc/ and the reference's obs-*.txt.
// -ppc-orig (opt.orig) in that of an -orig fit: gamma.txt / beta.txt; pi is drawn per replicate, B is the fit's point
// estimate.
// 0, or -1 with a message on stderr; throws SvilsError where a svils_ppc_* call fails
int run_ppc(Env &env, Network &network, const PpcOptions &opt);
// -gen: gen/network_gen.dat, gen/pi-gen.txt, gen/beta-gen.txt (MMSBGen::gen, save_model)
int run_gen(uint32_t n, uint32_t k, uint32_t seed, int device);

}  // namespace svinet
