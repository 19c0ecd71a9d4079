// Host driver of tpp-mlir_amd/csrc/rt_relayout.h for tests/test_relayout_decompose.py: reads "op esz m n ldi ldo N" and N lines
// "in out" (byte addresses) from stdin, prints the number of runs (-1: not a set of runs) and one line per run.
#include "rt_relayout.h"
#include <cstdio>

int main() {
  long long op, esz, m, n, ldi, ldo, N;
  if (scanf("%lld %lld %lld %lld %lld %lld %lld", &op, &esz, &m, &n, &ldi, &ldo, &N) != 7) return 2;
  std::vector<tpp::RelayoutItem> items((size_t)N);
  for (auto &it : items) {
    unsigned long long a, b;
    if (scanf("%llu %llu", &a, &b) != 2) return 2;
    it.in = (uintptr_t)a, it.out = (uintptr_t)b;
  }
  tpp::RelayoutRun runs[tpp::RELAYOUT_MAX_RUNS];
  const int nr = tpp::relayout_decompose(op, (int)esz, m, n, ldi, ldo, items, runs, tpp::RELAYOUT_MAX_RUNS);
  printf("%d\n", nr);
  for (int k = 0; k < nr; ++k)
    printf("%llu %llu %d %d %lld %lld %lld %lld %d\n", (unsigned long long)(uintptr_t)runs[k].in, (unsigned long long)(uintptr_t)runs[k].out,
           runs[k].R, runs[k].C, (long long)runs[k].in_r, (long long)runs[k].in_c, (long long)runs[k].out_r, (long long)runs[k].out_c, runs[k].vec);
  return 0;
}
