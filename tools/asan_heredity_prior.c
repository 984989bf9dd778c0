/* The host driver's heredity scalars under AddressSanitizer + UBSan, as a stand-alone program on the lnL = 0 back-end (no GPU,
 * no Python): 12 four-tip loci with a theta prior and a root-tau prior, so that THETA / TAU / MIX take their sums of T2h/h_i;
 * fixed scalars (cycling 1 / 0.75 / 0.25) and estimated ones (HRDT on, gamma(4, 4)); both proposal kernels, BPP's with the
 * program's moves; two threads; 300 iterations each.  Build and run from the repository root (libbpp_amd.so must have been
 * built):
 *
 *   gcc -O1 -g -std=c99 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer -I include \
 *       tools/asan_heredity_prior.c bpp_amd/csrc/host/a00_driver.c -o /tmp/asan_heredity_prior \
 *       -L bpp_amd -lbpp_amd -Wl,-rpath,$PWD/bpp_amd -lm && /tmp/asan_heredity_prior
 */
#include <stdio.h>
#include <stdlib.h>
#include "bpp_amd_host.h"

int main(void)
{
  enum { L = 12 };
  /* ((A,B),C),D: species tree of four species, caterpillar gene trees above the divergences */
  const int sp_parent[7] = { 4, 4, 5, 6, 5, 6, -1 };
  const double tau[7] = { 0, 0, 0, 0, 0.001, 0.002, 0.003 }, theta[7] = { 0.002, 0.002, 0.002, 0.002, 0.002, 0.002, 0.002 };
  const int left[7] = { -1, -1, -1, -1, 0, 4, 5 }, right[7] = { -1, -1, -1, -1, 1, 2, 3 };
  static const double cycle[3] = { 1.0, 0.75, 0.25 };
  int kernel, est, it; unsigned i;
  for (kernel = 0; kernel < 2; ++kernel)
    for (est = 0; est < 2; ++est)
    {
      a00_driver_t * d = a00_create(L, a00_backend_prior, NULL, 17);
      double h[L], h0[L], bad[L]; unsigned long prop, acc; int moved = 0;
      a00_set_proposal_kernel(d, kernel);
      if (kernel) a00_set_program_moves(d, 1, 0.3);
      a00_set_threads(d, 2);
      for (i = 0; i < L; ++i)
      {
        const double times[7] = { 0, 0, 0, 0, 0.0015 + 1e-5*i, 0.0025, 0.004 };
        if (!a00_set_tree(d, i, 4, left, right, times, 6, 0)) return 1;
        h0[i] = cycle[i % 3]; bad[i] = 1.0;
      }
      if (!a00_set_species_tree(d, 4, sp_parent, tau, theta)) return 2;
      a00_set_tau_prior(d, 3.0, 1000.0);
      a00_set_theta_prior(d, 2.0, 1000.0, 0.001);
      bad[L - 1] = 0.0;
      if (a00_set_heredity(d, bad)) return 3;                          /* refused: a scalar of 0 */
      if (!a00_set_heredity(d, h0)) return 4;
      if (a00_set_heredity_move(d, 1.0, 0.0, 4.0)) return 5;           /* refused: a = 0 with the move on */
      if (!a00_set_heredity_move(d, est ? 1.0 : 0.0, 4.0, 4.0)) return 6;
      if (!a00_initialize(d)) return 7;
      if (a00_set_heredity(d, h0)) return 8;                           /* refused: after the start-up densities */
      for (it = 0; it < 300; ++it) if (!a00_iterate(d)) return 9;
      a00_get_heredity(d, h);
      a00_heredity_counters(d, &prop, &acc);
      for (i = 0; i < L; ++i) { moved += h[i] != h0[i]; if (!(h[i] > 0)) return 10; }
      printf("kernel %d, scalars %s: HRDT %lu/%lu, h_0 %.6f, h_1 %.6f\n", kernel, est ? "estimated" : "fixed", acc, prop, h[0], h[1]);
      if (prop != (est ? 300ul*L : 0ul) || (est ? !(acc > 0 && acc < prop && moved) : (acc != 0 || moved))) return 11;
      a00_destroy(d);
    }
  printf("ok\n");
  return 0;
}
