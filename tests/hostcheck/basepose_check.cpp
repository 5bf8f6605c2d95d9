// basepose_check.cpp -- prints er::frag_basepose(length) (csrc/er_mat4.h) as the 16 bit patterns of its float64 entries, one per line, for
// tests/test_fragments_cpu.py to compare with synth.basepose.
#include "er_mat4.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char** argv) {
  const double length = argc > 1 ? strtod(argv[1], nullptr) : 3.0;
  double M[16];
  er::frag_basepose(length, M);
  for (int i = 0; i < 16; i++) {
    uint64_t u;
    memcpy(&u, &M[i], sizeof u);
    printf("%016llx\n", (unsigned long long)u);
  }
  return 0;
}
