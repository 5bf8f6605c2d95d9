// compact_check -- csrc/er_compact.h on its own: the host's prefix over block counts, the lists of a two-pass call, and the block helper of the
// kernels.  Without a HIP device the prefix arithmetic and the allocation-failure path are checked (nobody reaches the GPU); with one, a small
// kernel of this file drives the block helper through both passes and a host loop restates it.  Built from this file and csrc/er_common.cpp
// alone; prints one line per check and exits non-zero at the first that fails, so nothing is started after a HIP error.
#include "er_compact.h"

#include "er_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

void check(bool ok, const char* what) {
  printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
  fflush(stdout);
  if (!ok) exit(1);
}

bool says(const char* text) { return strstr(er_last_error(), text) != nullptr; }

void prefix_function() {
  long off[4] = {-7, -7, -7, -7};
  const long none = 0;
  check(er::exclusive_offsets(&none, 0, 1, off) == 0 && off[0] == -7, "n = 0: total 0, nothing written");
  const long one = 5;
  check(er::exclusive_offsets(&one, 1, 1, off) == 5 && off[0] == 0 && off[1] == -7, "n = 1: offset 0, total = the count");
  const long c[9] = {3, 100, 200, 0, 101, 201, 4, 102, 202};
  check(er::exclusive_offsets(c, 4, 1, off) == 303 && off[0] == 0 && off[1] == 3 && off[2] == 103 && off[3] == 303, "stride 1");
  check(er::exclusive_offsets(c, 4, 2, off) == 3 + 200 + 101 + 4 && off[1] == 3 && off[2] == 203 && off[3] == 304, "stride 2");
  check(er::exclusive_offsets(c, 3, 3, off) == 7 && off[0] == 0 && off[1] == 3 && off[2] == 3, "stride 3: every third count, a zero among them");
  const long big[3] = {1L << 30, 1L << 30, 1L << 30};
  check(er::exclusive_offsets(big, 3, 1, off) == 3L << 30 && off[2] == 1L << 31, "a total above 2^31 stays exact (long throughout)");
}

void two_lists() {
  er::TwoPass t;
  check(t.empty(), "a fresh object is empty");
  const int a = t.add(3, 3), b = t.add(2, 1), z = t.add(0, 2);
  check(a == 0 && b == 1 && z == 2 && !t.empty(), "three lists, the last without a block");
  const long ca[9] = {3, 1, 0, 0, 2, 2, 4, 0, 1}, cb[2] = {1L << 31, 9};
  memcpy(t.host_counts(a), ca, sizeof ca);
  memcpy(t.host_counts(b), cb, sizeof cb);
  t.prefix();
  const long *oa = t.host_offsets(a), *ob = t.host_offsets(b);
  check(oa[0] == 0 && oa[1] == 3 && oa[2] == 3 && t.total(a) == 7, "list 0: offsets and total over its first tally, stride 3");
  check(t.total(a, 1) == 3 && t.total(a, 2) == 3, "list 0: the sums of its two side tallies");
  check(ob[0] == 0 && ob[1] == 1L << 31 && t.total(b) == (1L << 31) + 9, "list 1: its own offsets from 0, a total above 2^31");
  check(t.total(z) == 0 && t.total(z, 1) == 0, "a list without a block: 0 and 0");
  check(t.host_counts(b) == t.host_counts(a) + 9 && ob == oa + 3, "the lists lie behind each other: [tallies * b + q] counts, [b] offsets");
}

void alloc_fails() {
  er::TwoPass t;
  er::DevScope scope;
  t.add(3, 2);
  t.add(1, 1);
  check(t.alloc(scope, "compact_who") == 1, "a failed alloc returns 1");
  check(t.empty(), "and leaves the object empty");
  check(says("compact_who") && says("hipMalloc(88 bytes)"), "its error text names the caller, the call and the size (7 counts + 4 offsets)");
  check(t.add(2, 1) == 0, "the object can be declared on again: the next list is list 0");
}

// One element per thread: bit 0 of flag[i] is the predicate that compacts, bits 1 and 2 the side tallies.
template <int N>
__global__ __launch_bounds__(256) void k_two_pass(const int* __restrict__ flag, long n, long* __restrict__ blk, const long* __restrict__ off, int pass,
                                                  int* __restrict__ rank_out, int* __restrict__ out) {
  __shared__ int s_tally[N][256 / 64];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool pred[N];
  for (int q = 0; q < N; q++) pred[q] = i < n && ((flag[i] >> q) & 1);
  const er::BlockTally<256, N> tally(s_tally, pred);
  if (!pass) {
    tally.block_totals(blk);
    return;
  }
  if (i >= n) return;
  rank_out[i] = (int)tally.rank_in_block();
  if (pred[0]) out[tally.rank_in_block(off[blockIdx.x])] = (int)i;
}

template <int N>
void both_passes(long n, bool all_kept) {
  char what[160];
  snprintf(what, sizeof what, "%d tall%s, n = %ld, %s", N, N == 1 ? "y" : "ies", n, all_kept ? "all kept" : "every third kept");
  std::vector<int> flag((size_t)n), rank((size_t)n, -1), out((size_t)n, -1);
  for (long i = 0; i < n; i++) flag[(size_t)i] = (all_kept || i % 3 == 0 ? 1 : 0) | (i % 2 == 0 ? 2 : 0) | (i % 5 == 0 ? 4 : 0);
  const long nblk = (n + 255) / 256;
  er::TwoPass t;                                               // (outlives the scope; the stream is synchronised before either goes)
  er::DevScope scope;
  const int l = t.add(nblk, N);
  int *d_flag = nullptr, *d_rank = nullptr, *d_out = nullptr;
  bool ok = t.alloc(scope, "compact_check") == 0 && scope.alloc(&d_flag, (size_t)n, "compact_check") == 0 &&
            scope.alloc(&d_rank, (size_t)n, "compact_check") == 0 && scope.alloc(&d_out, (size_t)n, "compact_check") == 0;
  if (!ok) check(false, what);
  auto launch = [&](int pass) {
    if (nblk == 0) return true;                                // (nothing to launch: the host half alone)
    hipLaunchKernelGGL(k_two_pass<N>, dim3((unsigned)nblk), dim3(256), 0, nullptr, d_flag, n, t.blk(l), t.off(l), pass, d_rank, d_out);
    return hipGetLastError() == hipSuccess;
  };
  ok = (n == 0 || hipMemcpyAsync(d_flag, flag.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, nullptr) == hipSuccess) && launch(0) &&
       t.read_counts("compact_check", nullptr) == 0 && hipStreamSynchronize(nullptr) == hipSuccess;
  if (!ok) check(false, what);
  t.prefix();
  // the host loop: counts per block, ranks inside a block, the sums, the order
  long kept = 0, side[3] = {0, 0, 0};
  std::vector<int> want_rank((size_t)n), want_out;
  for (long b = 0; b < nblk; b++) {
    long c[3] = {0, 0, 0};
    for (long i = 256 * b; i < n && i < 256 * (b + 1); i++) {
      want_rank[(size_t)i] = (int)c[0];
      if (flag[(size_t)i] & 1) want_out.push_back((int)i);
      for (int q = 0; q < N; q++) c[q] += (flag[(size_t)i] >> q) & 1;
    }
    ok = ok && t.host_offsets(l)[b] == kept;
    for (int q = 0; q < N; q++) ok = ok && t.host_counts(l)[N * b + q] == c[q];
    kept += c[0];
    for (int q = 1; q < N; q++) side[q] += c[q];
  }
  ok = ok && t.total(l) == kept;
  for (int q = 1; q < N; q++) ok = ok && t.total(l, q) == side[q];
  if (!ok) check(false, what);
  ok = t.upload_offsets("compact_check", nullptr) == 0 && launch(1) &&
       (n == 0 || (hipMemcpyAsync(rank.data(), d_rank, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, nullptr) == hipSuccess &&
                   hipMemcpyAsync(out.data(), d_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, nullptr) == hipSuccess)) &&
       hipStreamSynchronize(nullptr) == hipSuccess;
  if (!ok) check(false, what);
  ok = rank == want_rank && (long)want_out.size() == kept;
  for (long j = 0; j < kept; j++) ok = ok && out[(size_t)j] == want_out[(size_t)j];
  check(ok, what);
}

void with_device() {
  check(hipSetDevice(0) == hipSuccess, "hipSetDevice(0)");
  const long sizes[9] = {0, 1, 63, 64, 65, 255, 256, 257, 513};
  for (long n : sizes)
    for (int all_kept = 0; all_kept < 2; all_kept++) {
      both_passes<1>(n, all_kept != 0);
      both_passes<3>(n, all_kept != 0);
    }
}

}  // namespace

int main() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    printf("no device: checking the prefix and the failure path\n");
    prefix_function();
    two_lists();
    alloc_fails();
  } else {
    printf("%d device(s): checking both passes on the card\n", n);
    prefix_function();
    two_lists();
    with_device();
  }
  printf("OK\n");
  return 0;
}
