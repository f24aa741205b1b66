// plan_dump.cpp — prints ntt_plan (csrc/ntt_plan.hpp) for logn 1..28, both
// directions and 1 and 8 batches (TEST ONLY; compiled with the host compiler and
// run by tests/test_ntt_plan.py). One line per pass:
//   logn dit batches pass K s0 lo threads small
#include <cstdio>

#include "../../zk_stark_project_amd/csrc/ntt_plan.hpp"

int main() {
  const uint32_t batch_counts[] = {1, 8};
  for (uint32_t logn = 1; logn <= 28; logn++)
    for (int dit = 0; dit < 2; dit++)
      for (uint32_t batches : batch_counts) {
        const NttPlan pl = ntt_plan(logn, dit != 0, batches);
        for (uint32_t p = 0; p < pl.n; p++) {
          const NttPass& ps = pl.pass[p];
          printf("%u %d %u %u %u %u %u %u %d\n", logn, dit, batches, p, ps.K, ps.s0, ps.lo, 1u << ps.lognt,
                 ps.small ? 1 : 0);
        }
      }
  return 0;
}
