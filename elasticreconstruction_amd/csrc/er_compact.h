// er_compact.h -- ordered (stable) stream compaction in two passes, stated once.  A kernel runs twice over the same blocks: pass 0
// counts what each block keeps, the host turns the counts into exclusive offsets, pass 1 writes every kept element at its block's offset plus its
// rank inside the block: the output is in input order whatever the schedule.  Device half: the ballot / popcount / LDS part of such a kernel; host
// half: the arrays between the passes and who owns them.  Internal, no translation unit of its own; needs only er_common.h and er_mem.h.
#pragma once

#include "er_common.h"
#include "er_mem.h"

#include <vector>

namespace er {

#ifdef __HIPCC__
// The set bits of a wave's ballot below `lane`: the rank of this lane's element among those the wave keeps.
__device__ __forceinline__ int wave_rank(unsigned long long ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// x summed over lanes 0 .. lane of the wave (every lane calls it): where a lane keeps a COUNT of elements, not one -- its elements start at this
// minus its own x, and lane 63 holds the wave's total.
__device__ __forceinline__ int wave_inclusive_sum(int x, int lane) {
  for (int sft = 1; sft < 64; sft <<= 1) {
    const int t = __shfl_up(x, sft);
    if (lane >= sft) x += t;
  }
  return x;
}

// N predicates per thread of a kBlock-thread block (one element per thread, in thread order), tallied per block: the first is the one that
// compacts, the others are side tallies that ride along.  EVERY thread of the block reaches the constructor -- it holds the kernel's one
// __syncthreads() -- so a thread without an element comes with all-false predicates, and the kernel's early returns stand behind it.
// lds: the caller's __shared__ int [N][kBlock / 64], used by nothing else.
template <int kBlock, int N>
class BlockTally {
  static_assert(kBlock % 64 == 0 && N >= 1 && N <= 3, "whole waves, one to three tallies");

 public:
  __device__ __forceinline__ BlockTally(int (&lds)[N][kBlock / 64], const bool (&pred)[N]) : s_(lds), lane_(threadIdx.x & 63), w_(threadIdx.x >> 6) {
    unsigned long long b[N];
#pragma unroll
    for (int q = 0; q < N; q++) b[q] = __ballot(pred[q]);
    if (lane_ == 0) {
#pragma unroll
      for (int q = 0; q < N; q++) s_[q][w_] = __popcll(b[q]);
    }
    first_ = b[0];
    __syncthreads();
  }
  // Pass 0: thread 0 writes the block's N totals to blk[N * blockIdx.x + q] (TwoPass::blk of a list with N tallies).
  __device__ __forceinline__ void block_totals(long* __restrict__ blk) const {
    if (threadIdx.x != 0) return;
    long t[N] = {};
    for (int w = 0; w < kBlock / 64; w++)
#pragma unroll
      for (int q = 0; q < N; q++) t[q] += s_[q][w];
#pragma unroll
    for (int q = 0; q < N; q++) blk[N * (long)blockIdx.x + q] = t[q];
  }
  // Pass 1: base + how many threads below this one have their first predicate set.  The element goes to rank_in_block(off[blockIdx.x]).
  __device__ __forceinline__ long rank_in_block(long base = 0) const {
    long r = base + wave_rank(first_, lane_);
    for (int q = 0; q < w_; q++) r += s_[0][q];
    return r;
  }

 private:
  int (&s_)[N][kBlock / 64];
  const int lane_, w_;
  unsigned long long first_;
};
#endif  // __HIPCC__

// n counts, `stride` apart, into n exclusive offsets (offsets == NULL: none are written); returns their total.
__attribute__((visibility("hidden"))) inline long exclusive_offsets(const long* counts, long n, long stride, long* offsets) {
  long total = 0;
  for (long b = 0; b < n; b++) {
    if (offsets) offsets[b] = total;
    total += counts[stride * b];
  }
  return total;
}

// What stands between the two passes of one call, for every list it compacts.  The call declares its lists -- add(blocks, tallies per block) --
// and allocates once; a list's kernel gets blk(list) = its counts [tallies * b + q] and off(list) = its offsets [b].  Then, in this order: the
// count launches, read_counts, the CALLER's stream synchronise (nothing here synchronises), prefix, upload_offsets, the write launches.  The
// host copies live here because the copies use them until the stream has run them: the object is kept where it outlives them -- in the result
// the call hands back or in the call's frame, and declared BEFORE the DevScope, whose hipFree waits for the stream on every way out.
class __attribute__((visibility("hidden"))) TwoPass {
 public:
  int add(long n_blocks, int tallies) {        // -> the list's index.  Before alloc.
    lists_.push_back(List{n_blocks, (long)h_cnt_.size(), (long)h_off_.size(), tallies, {0, 0, 0}});
    h_cnt_.resize(h_cnt_.size() + (size_t)(n_blocks * tallies), 0);
    h_off_.resize(h_off_.size() + (size_t)n_blocks, 0);
    return (int)lists_.size() - 1;
  }
  // One device allocation in `scope` for all counts and offsets.  On failure (returns 1, er::fail has the text) the object is empty again.
  int alloc(DevScope& scope, const char* who) {
    const int rc = scope.alloc(&d_, h_cnt_.size() + h_off_.size(), who);
    if (rc) *this = TwoPass();
    return rc;
  }
  bool empty() const { return !d_ && lists_.empty(); }
  long* blk(int list) const { return d_ + lists_[(size_t)list].cnt_at; }
  const long* off(int list) const { return d_ + h_cnt_.size() + lists_[(size_t)list].off_at; }
  long* host_counts(int list) { return h_cnt_.data() + lists_[(size_t)list].cnt_at; }
  const long* host_offsets(int list) const { return h_off_.data() + lists_[(size_t)list].off_at; }
  int read_counts(const char* who, hipStream_t s) {           // enqueues the one copy of all counts to the host
    if (!h_cnt_.empty()) ER_W(who, hipMemcpyAsync(h_cnt_.data(), d_, h_cnt_.size() * sizeof(long), hipMemcpyDeviceToHost, s));
    return 0;
  }
  void prefix() {                                              // once the stream has been synchronised: every list's offsets and tally sums
    for (List& l : lists_)
      for (int q = 0; q < l.tallies; q++)
        l.sum[q] = l.n ? exclusive_offsets(h_cnt_.data() + l.cnt_at + q, l.n, l.tallies, q ? nullptr : h_off_.data() + l.off_at) : 0;
  }
  // Tally 0: how many elements the list keeps; the others: the sum of that side tally.
  long total(int list, int tally = 0) const { return lists_[(size_t)list].sum[tally]; }
  int upload_offsets(const char* who, hipStream_t s) {        // enqueues the one copy of all offsets to the device
    if (!h_off_.empty()) ER_W(who, hipMemcpyAsync(d_ + h_cnt_.size(), h_off_.data(), h_off_.size() * sizeof(long), hipMemcpyHostToDevice, s));
    return 0;
  }

 private:
  struct List {
    long n, cnt_at, off_at;
    int tallies;
    long sum[3];
  };
  std::vector<List> lists_;
  long* d_ = nullptr;                          // [h_cnt_.size()] counts, then [h_off_.size()] offsets: the scope's
  std::vector<long> h_cnt_, h_off_;
};

}  // namespace er
