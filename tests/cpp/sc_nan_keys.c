/* orc_sc_detect on a database that holds non-finite ring keys -- a stand-alone program for a sanitizer build of the oracle
 * (tests/test_scancontext_shapes.py).  The rule (randt_oracle.h): an entry whose float key distance to the query is not >= 0
 * is never a candidate; when no candidate is left the remaining ranks are absent. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "randt_oracle.h"

#define N_DB 40
#define R 20
#define S 45

int main(void) {
  orc_sc_params p = {R, S, 15.0, 15, 10, 0.3, 0.3, 0.05, 1.2, 0.0, 0.04};
  double* desc = (double*)calloc((size_t)N_DB * S * R, sizeof(double));
  double* rk = (double*)calloc((size_t)N_DB * R, sizeof(double));
  double pos[2 * N_DB], dist[N_DB];
  unsigned seed = 12345u;
  for (int i = 0; i < N_DB; ++i) {
    for (int b = 0; b < S * R; ++b) {
      seed = seed * 1664525u + 1013904223u;
      if ((seed >> 24) % 3 == 0) desc[(size_t)i * S * R + b] = 1 + (seed >> 16) % 8;
    }
    pos[2 * i] = 0.3 * i;
    pos[2 * i + 1] = 0.1 * (i % 7);
    dist[i] = 0.5 * (i + 1);
  }
  const int nan_nodes[3] = {2, 30, 31};
  for (int k = 0; k < 3; ++k) desc[(size_t)nan_nodes[k] * S * R + 5 * R + 3] = NAN;
  desc[(size_t)7 * S * R + 2 * R + 1] = INFINITY; /* an infinite key: distance +inf to a finite query (a candidate like any other), NaN to itself */
  for (int i = 0; i < N_DB; ++i)
    for (int r = 0; r < R; ++r) {
      double a = 0;
      for (int s = 0; s < S; ++s) a += desc[(size_t)i * S * R + (size_t)s * R + r];
      rk[(size_t)i * R + r] = a / S;
    }
  int bad = 0;
  for (int q = 0; q <= N_DB; ++q) { /* N_DB itself: the early return */
    float yaw = -1.0f;
    double md = -1.0;
    const int id = orc_sc_detect(&p, desc, rk, pos, dist, N_DB, q, &yaw, &md);
    if (id == 2 || id == 30 || id == 31 || id >= N_DB || id < -1 || !(md >= 0)) ++bad;
    if ((q == 30 || q == 31) && (id != -1 || md != 10000000 || yaw != 0.0f)) ++bad; /* a NaN query has no candidate */
    if (q == 16 && id != -1 && id != 0) ++bad;                                    /* searchable: node 0 and 1 only */
  }
  free(desc);
  free(rk);
  if (bad) {
    printf("FAILED: %d queries\n", bad);
    return 1;
  }
  printf("ok\n");
  return 0;
}
