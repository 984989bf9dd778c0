/* The host driver's locus-rate moves under AddressSanitizer + UBSan, as a stand-alone program on the lnL = 0 back-end (no
 * GPU, no Python): 12 four-tip loci, MUI + MUBAR on (a_mui = 5, mubar ~ gamma(10, 10)), then mubar fixed; both proposal
 * kernels; 300 iterations each.  Build and run from the repository root (libbpp_amd.so must have been built):
 *
 *   gcc -O1 -g -std=c99 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer -I include \
 *       tools/asan_locusrate_prior.c bpp_amd/csrc/host/a00_driver.c -o /tmp/asan_locusrate_prior \
 *       -L bpp_amd -lbpp_amd -Wl,-rpath,$PWD/bpp_amd -lm && /tmp/asan_locusrate_prior
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
  int kernel, fixed, it; unsigned i;
  for (kernel = 0; kernel < 2; ++kernel)
    for (fixed = 0; fixed < 2; ++fixed)
    {
      a00_driver_t * d = a00_create(L, a00_backend_prior, NULL, 17);
      double mui[L], mubar, bad[L]; unsigned long prop[2], acc[2];
      a00_set_proposal_kernel(d, kernel);
      for (i = 0; i < L; ++i)
      {
        const double times[7] = { 0, 0, 0, 0, 0.0015 + 1e-5*i, 0.0025, 0.004 };
        if (!a00_set_tree(d, i, 4, left, right, times, 6, 0)) return 1;
        mui[i] = 0.5 + 0.1*i; bad[i] = 1.0;
      }
      if (!a00_set_species_tree(d, 4, sp_parent, tau, theta)) return 2;
      bad[L - 1] = 0.0;
      if (a00_set_locus_rates(d, bad)) return 3;                       /* refused: a rate of 0 */
      if (!a00_set_locus_rates(d, mui)) return 4;
      if (a00_set_locusrate_moves(d, 1.2, 0.6, 0.0, 10.0, 10.0, 1.0)) return 5;      /* refused: a_mui = 0 with a move on */
      if (!a00_set_locusrate_moves(d, 1.2, 0.6, 5.0, fixed ? 0.0 : 10.0, fixed ? 0.0 : 10.0, 1.0)) return 6;
      if (!a00_initialize(d)) return 7;
      if (a00_set_locus_rates(d, mui)) return 8;                       /* refused: after the start-up evaluation */
      for (it = 0; it < 300; ++it) if (!a00_iterate(d)) return 9;
      a00_get_locus_rates(d, mui, &mubar);
      a00_locusrate_counters(d, prop, acc);
      printf("kernel %d, mubar %s: MUI %lu/%lu, MUBAR %lu/%lu, mubar %.6f, mu_0 %.6f\n", kernel, fixed ? "fixed" : "moved", acc[0], prop[0], acc[1], prop[1], mubar, mui[0]);
      if (prop[0] != 300ul*L || prop[1] != (fixed ? 0ul : 300ul) || !(mubar > 0)) return 10;
      a00_destroy(d);
    }
  printf("ok\n");
  return 0;
}
