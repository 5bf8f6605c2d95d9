// er_tsdf.hip -- path A of liber_hip.so: TSDF depth integration with control-grid warp on MI355X
// (gfx950).  Replaces the reference's TSDFVolume / TSDFVolumeUnit / ControlGrid / CIntegrateApp::Reproject
// (Integrate/TSDFVolume.cpp:19-132, TSDFVolumeUnit.cpp:4-21, ControlGrid.h:41-87, IntegrateApp.cpp:228-269).
//
// Data layout in HBM (one er_tsdf_s per GPU):
//   pool      float2[max_units][64][64][64]   {sdf_, weight_} interleaved per voxel, k fastest
//                                             (the reference keeps two float[64^3] per unit,
//                                             TSDFVolumeUnit.h:108-109; interleaving makes the
//                                             read-modify-write one 8-byte access per voxel)
//   ht_*      open-addressing hash map  hash_key -> {pool slot, 64-bit frame mask}; the device-side
//                                             twin of TSDFVolume::data_ (TSDFVolume.h:27)
//   lambda    float[rows*cols]                ScaleDepth's per-pixel ray-length factor (camera constant)
//   scaled    float[64][rows*cols]            scaled depth of every frame of the batch in flight
//   zbuf      uint32[64][rows*cols]           Reproject's z-buffer (atomicMin of epoch tag | depth, er_tsdf.h: kZEpochMax; a cell without the
//                                             current tag is empty); lastzero / zfix: its replay state
//
// Launch sequence for a batch of <= 64 frames (er_tsdf_integrate_frames); three batches are in flight (run_batch):
//  pre-pass stream (batch b on stream b mod 2):
//   [k_reproject_scatter -> k_reproject_fix]          per SOURCE pixel: warp + scatter-min   (A6/A7)
//   k_prepare      per pixel: ScaleDepth + unit key; marks bit f in the unit's frame mask,   (A3/A5)
//                  appends the unit to the batch list
//   k_plan         hands new units their pool slots, writes one record {key, slot, frame mask} per unit of the batch in cost order
//                  (frames in the mask) and resets the work queue k_integrate claims its items from; clears the frame masks and
//                  the list behind its copies
//  main stream:
//   k_integrate    per wave an 8 x 4 x 8 box of a unit: each voxel is loaded ONCE, run against every (A4)
//                  frame whose bit is set IN FRAME ORDER, stored once -> bit-identical to the reference's
//                  frame-by-frame loop with 1/batch of its HBM traffic
// All kernels are HBM/latency/VALU work on scattered voxels and pixels: no MFMA.
//
// The pre-pass kernels and the voxel pass are compiled in files of their own (er_tsdf_pre.hip, er_tsdf_int.hip; er_tsdf.h says why), the extraction
// and the band records of the multi-GPU merge live in er_tsdf_extract.hip and er_tsdf_band.hip.
#include "er_tsdf_dev.h"

#include <chrono>
#include <climits>

namespace {

using namespace er_tsdf_k;

constexpr int kNbatchSlot[3] = {C_NBATCH, C_NBATCH1, C_NBATCH2};
constexpr int kZeroFlagSlot[2] = {C_ZERO_WRITE, C_ZERO_WRITE1};

// ------------------------------------------------------------------------------------------------
// ScaleDepth's camera-constant factor (TSDFVolume.cpp:24-26), tabulated once per volume.
__global__ void k_lambda(float* __restrict__ lambda, int cols, int rows, Camera cam) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= cols * rows) return;
  lambda[p] = scale_lambda(p % cols, p / cols, cam);
}

// Stand-alone ScaleDepth (TSDFVolume.cpp:19-36) for er_tsdf_scale_depth.
__global__ void k_scale_depth(const uint16_t* __restrict__ depth, const float* __restrict__ lambda,
                              float* __restrict__ scaled, int pixels, float itrunc) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  scaled[p] = scale_depth_px(depth[p], lambda[p], itrunc);
}

// The order-dependent case (a write of dd == 0 resets the cell: "0 means empty"), replayed exactly.  ONE launch of kFixBlocks
// single-wave workgroups that return at once unless a frame of the batch is flagged -- practically never -- and otherwise share the
// pixels of the flagged frames: every source pixel is warped again and scattered into zfix under the replay rule.  One phase, no
// ordering between workgroups; the consumer merges (take_z, er_tsdf_dev.h) and re-arms lastzero / zfix (plain depths, no epoch tag), k_plan (or the single-frame entry
// point) clears the flag words.  Single-wave workgroups with a capped register budget: they find a free wave slot at once next to the
// persistent k_integrate workgroups (a 256-thread workgroup waited 46 us on average for four slots on one CU).
__global__ __launch_bounds__(kFixThreads) __attribute__((amdgpu_num_vgpr(48))) void k_reproject_fix(ReprojArgs A) {
  const int fl0 = A.zero_flag[0], fl1 = A.zero_flag[1];
  if ((fl0 | fl1) == 0) return;
  const int pixels = A.cols * A.rows;
  for (int f = 0; f < A.n_frames; f++) {
    if ((((f < 32 ? fl0 : fl1) >> (f & 31)) & 1) == 0) continue;
    for (int p = blockIdx.x * kFixThreads + threadIdx.x; p < pixels; p += gridDim.x * kFixThreads) reproject_scatter_px(A, f, p % A.cols, p / A.cols, 1);
  }
}

__global__ void k_zbuf_to_depth(const uint32_t* __restrict__ zbuf, uint16_t* __restrict__ depth, long total, uint32_t* __restrict__ lastzero,
                                uint32_t* __restrict__ zfix, const int* __restrict__ zero_flag, uint32_t ztag) {
  long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  uint32_t z = z_of_epoch(zbuf[t], ztag);                               // (the z-buffer is not re-armed: its next use has another tag)
  if (zero_flag[0] & 1) z = take_z(z, (size_t)t, lastzero, zfix);       // (single frame: bit 0)
  depth[t] = (z == kZEmpty) ? (uint16_t)0 : (uint16_t)z;
}

// ------------------------------------------------------------------------------------------------
// Work plan of one batch (single workgroup; a batch touches at most a few hundred units): the units of the
// batch list sorted by DESCENDING cost = popcount(frame mask) -- the order in which the persistent workgroups of k_integrate
// claim their items from the work queue (longest-processing-time first) -- and the queue head reset to 0.

// Pool slot of hash entry e; hands the slot out on the unit's first ever visit (data_.find( key ) == end, TSDFVolume.cpp:55; pool
// memory is zero-filled up front).  Called by ONE thread per unit from k_plan.  The pre-passes of two batches run concurrently, so
// two k_plan launches can race for a new unit: one wins the compare-and-swap (-1 -> -2), draws the slot and publishes it; the
// other polls until it appears (the winner is a running thread of a resident single-workgroup kernel, so the wait is bounded).
// -3 = pool exhausted.  (Rounds 1-2 did this from k_integrate, per wave and item.)
// Two phases in program order -- winners draw and publish WITHOUT ever waiting, only then do the losers poll -- so that lanes of one
// wave that lost against the other launch cannot hold up lanes of the same wave that won (a wave runs the two sides of a divergent
// branch one after the other).
__device__ int unit_slot_acquire(int e, int key, int* __restrict__ ht_slot, int* __restrict__ unit_key, int max_units, int* __restrict__ counters) {
  int slot = __hip_atomic_load(&ht_slot[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  bool won = false;
  if (slot == -1) won = atomicCAS(&ht_slot[e], -1, -2) == -1;
  if (won) {
    const int s = atomicAdd(&counters[C_NUNITS], 1);
    if (s < max_units) {
      unit_key[s] = key;
      __threadfence();
      slot = s;
    } else {
      atomicOr(&counters[C_POOL_OVERFLOW], 1);
      slot = -3;
    }
    atomicExch(&ht_slot[e], slot);
  }
  if (!won && (slot == -1 || slot == -2)) {
    do {
      slot = __hip_atomic_load(&ht_slot[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slot == -2) __builtin_amdgcn_s_sleep(8);
    } while (slot == -2);
  }
  return slot;
}

//
// The launch is also the last reader of the slot's frame masks, unit list and list length (k_integrate works from the copies in plan_rec), so it
// hands them back empty to the slot's next k_prepare: each mask is cleared behind its copy, the unit visits (sum of popcounts) are accounted in
// stats[0], and the length is zeroed behind the last barrier, when every thread has read it.
__global__ __launch_bounds__(256) void k_plan(const int* __restrict__ batch, int* nbatch,
                                              unsigned long long* __restrict__ ht_mask, const int* __restrict__ ht_key,
                                              int* __restrict__ ht_slot, int* __restrict__ unit_key, int max_units,
                                              int* __restrict__ counters, PlanRec* __restrict__ plan_rec, Plan* __restrict__ plan,
                                              int* __restrict__ zero_flag, unsigned long long* __restrict__ stats) {
  __shared__ int hist[65];
  __shared__ int start[66];
  const int n = *nbatch;                            // <= hash capacity = size of plan_rec
  for (int t = threadIdx.x; t < 65; t += blockDim.x) hist[t] = 0;
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += blockDim.x) atomicAdd(&hist[__popcll(ht_mask[batch[t]])], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int c = 64; c >= 0; c--) {                 // descending cost
      start[c] = acc;
      acc += hist[c];
    }
    plan->n_units = n;
    plan->next = 0;
    if (zero_flag) zero_flag[0] = zero_flag[1] = 0;     // Reproject's replay flags of this batch: consumed by the k_prepare in front of this launch
  }
  __syncthreads();
  if (threadIdx.x == 0) *nbatch = 0;
  unsigned long long visits = 0;
  for (int t = threadIdx.x; t < n; t += blockDim.x) {
    const int e = batch[t];
    const unsigned long long mask = ht_mask[e];
    ht_mask[e] = 0ull;                                                  // (a unit stands once in the list: nobody reads this mask again)
    visits += (unsigned long long)__popcll(mask);
    const int key = ht_key[e];
    PlanRec r;
    r.key = key;
    r.slot = unit_slot_acquire(e, key, ht_slot, unit_key, max_units, counters);
    r.mask = mask;
    plan_rec[atomicAdd(&start[__popcll(mask)], 1)] = r;                 // position in descending cost order
  }
  if (visits) atomicAdd(&stats[0], visits);
}

// ------------------------------------------------------------------------------------------------
// Sum of weight_ (= number of voxel updates, TSDFVolume.cpp:90,94); wave shuffle -> one atomic per block.
__global__ void k_sum_weight(const float2* __restrict__ pool, long n_vox, double* __restrict__ out) {
  double s = 0.0;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n_vox; t += (long)gridDim.x * blockDim.x)
    s += (double)pool[t].y;
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  __shared__ double part[kBlock / 64];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double b = 0.0;
    for (int w = 0; w < kBlock / 64; w++) b += part[w];
    atomicAdd(out, b);
  }
}

// Host-driven unit allocation (import of units this GPU never touched).
__global__ void k_ensure_units(const int* __restrict__ keys, int n, int* __restrict__ ht_key, int* __restrict__ ht_slot,
                               int cap_mask, int hash_shift, int* __restrict__ unit_key, int max_units,
                               int* __restrict__ counters, int* __restrict__ slots_out, int allocate) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int key = keys[t];
  int slot = -1;
  if (allocate) {
    const int e = ht_find_or_insert(ht_key, cap_mask, hash_shift, key);   // keys are unique: no race on the slot
    if (e < 0) {
      atomicOr(&counters[C_TABLE_FULL], 1);
    } else {
      slot = ht_slot[e];
      if (slot < 0) {
        const int s = atomicAdd(&counters[C_NUNITS], 1);
        if (s < max_units) {
          ht_slot[e] = s;
          unit_key[s] = key;
          slot = s;
        } else {
          atomicOr(&counters[C_POOL_OVERFLOW], 1);
        }
      }
    }
  } else {
    unsigned h = hash_unit_key(key, hash_shift);
    for (int probe = 0; probe <= cap_mask; ++probe) {
      const int e = (int)((h + (unsigned)probe) & (unsigned)cap_mask);
      const int k = ht_key[e];
      if (k == key) { slot = ht_slot[e]; break; }
      if (k == kEmptyKey) break;
    }
  }
  slots_out[t] = slot;
}

// n16 16-byte words and `tail` (< 4) 4-byte words behind them from a page-locked block of the handle, read in place, into device memory
// (fetch_pinned says why this is not a hipMemcpyAsync).  One load per thread for the per-batch constants; a grid-stride loop for more.
__global__ __launch_bounds__(kBlock) void k_fetch_pinned(const uint4* __restrict__ src, uint4* __restrict__ dst, int n16, int tail) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n16; i += gridDim.x * kBlock) dst[i] = src[i];
  if (blockIdx.x == 0 && (int)threadIdx.x < tail)
    reinterpret_cast<uint32_t*>(dst + n16)[threadIdx.x] = reinterpret_cast<const uint32_t*>(src + n16)[threadIdx.x];
}

}  // namespace

// ================================================================================================
hipStream_t er::tsdf_stream(er_tsdf_s* h) { return h->stream; }
int er::tsdf_device(er_tsdf_s* h) { return h->device; }

static int launch_reproject(er_tsdf_t h, const ReprojArgs& RA, int n, hipStream_t X);

namespace {

int drain_events(er_tsdf_t h) {
  for (auto& ev : h->events) {
    float ms = 0.f;
    ER_HIP_TRY(hipEventSynchronize(ev.second));
    ER_HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
    h->ms_total += ms;
    h->launches += 1;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  h->events.clear();
  return 0;
}

// The voxel passes run on own_stream (run_batch).  Whoever is about to use h->stream for the volume or its accounts -- check_flags,
// resolve_slots, the profile calls; sync_all waits for every stream: every entry point passes one of them before it touches the pool or
// the tables -- first makes a caller's stream wait for the last voxel pass, and with it for every pre-pass in front of it.  Lazily, not at the end of er_tsdf_integrate_frames: a wait parked in the caller's stream
// would hold up whatever shares its hardware queue, and the next call's "own_stream behind the caller's stream" would wait behind
// it for nothing (-1.4 % with 8 queues, profiles/r07a_timeline_queues.txt).
int join_voxel(er_tsdf_t h) {
  if (h->voxel_ahead) {
    ER_HIP_TRY(hipStreamWaitEvent(h->stream, h->voxel_done, 0));
    h->voxel_ahead = false;
  }
  return 0;
}

int ensure_key_scratch(er_tsdf_t h, size_t n) {
  if (n <= h->key_scratch.capacity()) return 0;
  const size_t cap = std::max<size_t>(n, 1024);
  if (h->key_scratch.reserve(cap, "the TSDF key scratch") || h->slot_scratch.reserve(cap, "the TSDF key scratch")) {
    h->key_scratch.reset();
    return 1;
  }
  return 0;
}

}  // namespace

namespace er_tsdf_k {

int check_flags(er_tsdf_t h) {
  int c[C_COUNT];
  if (join_voxel(h)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(c, h->counters, sizeof c, hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (c[C_POOL_OVERFLOW])
    return er::fail("TSDF unit pool exhausted: %d units requested, capacity %d (raise max_units)", c[C_NUNITS], h->max_units);
  if (c[C_TABLE_FULL]) return er::fail("TSDF unit hash table full (capacity %d)", h->ht_cap);
  return 0;
}

int next_ztag(er_tsdf_t h, int which, uint32_t* zbuf, size_t cells, hipStream_t X, uint32_t* ztag) {
  if (h->zepoch[which] >= kZEpochMax) {                                 // the next tag would fall below nothing: start over from an empty buffer
    ER_HIP_TRY(hipMemsetAsync(zbuf, 0xFF, cells * sizeof(uint32_t), X));
    h->zepoch[which] = 0;
  }
  h->zepoch[which]++;
  *ztag = (kZEpochMax - h->zepoch[which]) << 16;
  return 0;
}

// keys (host) -> slots (device slot_scratch), optionally allocating missing units.
int resolve_slots(er_tsdf_t h, const int* keys_host, int n, bool allocate) {
  if (join_voxel(h) || ensure_key_scratch(h, (size_t)n)) return 1;
  ER_HIP_TRY(hipMemcpyAsync(h->key_scratch, keys_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_ensure_units, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->key_scratch, n,
                     h->ht_key, h->ht_slot, h->ht_cap - 1, h->ht_shift, h->unit_key, h->max_units, h->counters,
                     h->slot_scratch, allocate ? 1 : 0);
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

int sorted_units(er_tsdf_t h, std::vector<int>& keys, std::vector<int>& slots) {
  if (check_flags(h)) return 1;
  int n = 0;
  ER_HIP_TRY(hipMemcpy(&n, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  n = std::min(n, h->max_units);
  std::vector<int> uk((size_t)n);
  if (n) ER_HIP_TRY(hipMemcpy(uk.data(), h->unit_key, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  std::vector<std::pair<int, int>> ks;
  ks.reserve((size_t)n);
  for (int s = 0; s < n; s++)
    if (!std::binary_search(h->dropped.begin(), h->dropped.end(), uk[(size_t)s])) ks.push_back(std::make_pair(uk[(size_t)s], s));   // (handed to their owner)
  std::sort(ks.begin(), ks.end());
  n = (int)ks.size();
  keys.resize((size_t)n);
  slots.resize((size_t)n);
  for (int s = 0; s < n; s++) {
    keys[(size_t)s] = ks[(size_t)s].first;
    slots[(size_t)s] = ks[(size_t)s].second;
  }
  return 0;
}

}  // namespace er_tsdf_k

namespace {

// Host staging layout of one batch's constants inside the pinned buffer of its parity.
struct Staging {
  er::FrameXform fx[ER_MAX_BATCH];
  float fxT[16][ER_MAX_BATCH];                     // the same constants component-major, DIRECTLY behind fx (k_integrate's culling reads them with lane = frame)
  double t12[ER_MAX_BATCH * 12];
  double seg[ER_MAX_BATCH * 16];
  double madj[ER_MAX_BATCH * 12];
  int gi[ER_MAX_BATCH];
};

// `bytes` (a multiple of 4) from a page-locked block of the handle (hipHostMalloc: mapped into the device's address space) to device memory,
// on stream s, by a kernel that reads the block in place.  Not hipMemcpyAsync: the runtime's host-to-device copy path stalls the calling
// thread for 5 - 9 ms a few times per process -- at copies number 8, 15 and about 25 of a fresh process and then once or twice more, at a
// moment that the timing of the first passes moves about -- and such a stall empties the pipeline, which runs 1.3 ms ahead of the device:
// one of them in a 3000-frame pass is 16 ms against 23 (profiles/r10a_slow_mode.txt).  A kernel launch takes the path of every other launch
// of the pipeline; what the host wrote before the launch is visible to the kernel, and the event recorded behind it frees the block.
int fetch_pinned(void* dst, void* pinned, size_t bytes, hipStream_t s) {
  void* src = nullptr;
  ER_HIP_TRY(hipHostGetDevicePointer(&src, pinned, 0));
  const size_t n16 = bytes / 16;
  if (bytes % 4 != 0 || n16 > (size_t)INT_MAX) return er::fail("fetch_pinned: %zu bytes", bytes);
  const int blocks = (int)std::min<size_t>(std::max<size_t>((n16 + kBlock - 1) / kBlock, 1), 64);
  hipLaunchKernelGGL(k_fetch_pinned, dim3(blocks), dim3(kBlock), 0, s, static_cast<const uint4*>(src), static_cast<uint4*>(dst), (int)n16,
                     (int)(bytes % 16 / 4));
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

double host_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// One timing event of a timeline row, recorded on s: an event of a row already read, or a new one.
int tl_record(er_tsdf_t h, hipEvent_t* e, hipStream_t s) {
  if (!h->tl_free.empty()) {
    *e = h->tl_free.back();
    h->tl_free.pop_back();
  } else {
    ER_HIP_TRY(hipEventCreate(e));
  }
  ER_HIP_TRY(hipEventRecord(*e, s));
  return 0;
}

// Waits for the rows' events and hands them back for re-use.
int tl_drop_rows(er_tsdf_t h) {
  for (auto& r : h->tl_rows)
    for (hipEvent_t e : r.ev)
      if (e) {
        ER_HIP_TRY(hipEventSynchronize(e));
        h->tl_free.push_back(e);
      }
  h->tl_rows.clear();
  return 0;
}

int sync_all(er_tsdf_t h) {
  if (h->copy_stream) ER_HIP_TRY(hipStreamSynchronize(h->copy_stream));
  for (int a = 0; a < kAux; a++) ER_HIP_TRY(hipStreamSynchronize(h->aux_stream[a]));
  if (h->stream != h->own_stream) ER_HIP_TRY(hipStreamSynchronize(h->own_stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  h->voxel_ahead = false;
  return 0;
}

// One batch (<= ER_MAX_BATCH frames).  depth_dev: n * pixels uint16 on device (must be complete: the
// pre-passes run on the handle's auxiliary streams, which do not wait for the caller's stream).
// Pipeline over three in-order streams.  Batch b owns pipeline slot p = b mod 3 and pre-pass stream X(b) = aux_stream[b mod 2]; V is
// the voxel stream (own_stream):
//   X(b): wait int_done[p] -> H2D constants(p) -> [k_reproject_scatter -> k_reproject_fix] -> k_prepare(p) -> k_plan(p) -> event pre_done[p]
//   V   : wait pre_done[p] -> k_integrate(p) -> event int_done[p]                          (ONE kernel per batch: it is the critical path)
// so the pre-passes of batches b+1 and b+2 (latency / float64 bound, each a serial chain of launches) overlap each other and
// k_integrate of batch b (float32 VALU bound): the two chains run staggered, one stream's scatter next to the other's k_prepare.
// Batches still reach the volume strictly in order (V).
//
// Who writes and reads what, for batches b, b+1, b+2 (b+3 is the next user of slot p, b+2 of stream X(b)):
//
//   buffer / flag word              written by                        read by                              what separates the next writer from them
//   ------------------------------  --------------------------------  -----------------------------------  ---------------------------------------------
//   pinned[p]            (host)     the host, batch b                 H2D constants(b) on X(b)             host waits consts_done[p] before batch b+3
//   dstage[p] = frames[p], t12,     H2D constants(b) on X(b), behind  scatter, fix, k_prepare(b) on X(b);  X(b+3) waits int_done[p] of b: recorded on V behind
//     seg, madj, gi                 int_done[p] of b-3                k_integrate(b) on V                  k_integrate(b), itself behind pre_done[p] of b
//   zbuf / lastzero / zfix [b mod   scatter(b), fix(b); lastzero and  k_prepare(b), all on X(b)            the next writer is scatter(b+2) on the same
//     2], zero-flag words [b mod 2] zfix re-armed by k_prepare(b),                                         stream, behind k_plan(b): stream order; zbuf is
//                                   the flags cleared by k_plan(b)                                         not re-armed: scatter(b+2) writes under the next
//                                                                                                          epoch's tag (next_ztag; a fill on X when it wraps)
//   depth_stage[p] (host frames)    frame copy(b) on the copy stream  scatter(b), k_prepare(b) on X(b),    copy(b+3) waits pre_done[p] of batch b, which
//                                   behind pre_done[p] of batch b-3   behind copy_done[p]                  k_plan(b) records behind both readers
//   ht_mask[p], batch[p], nbatch[p] k_prepare(b); cleared by          k_plan(b) on X(b), nobody else       k_prepare(b+3) on X(b+3) behind int_done[p] of b,
//                                   k_plan(b), its only reader        (k_integrate reads the mask from     hence behind k_plan(b)
//                                                                     plan_rec)
//   stats[0] (unit visits)          k_plan(b), atomically             er_tsdf_get_profile; cleared by      both on h->stream behind join_voxel: the last voxel
//                                                                     er_tsdf_set_profiling                pass stands behind every k_plan launched so far
//   scaled[p], tile_max / tile_lo   k_prepare(b) on X(b)              k_integrate(b) on V, behind          k_prepare(b+3) on X(b+3) behind int_done[p] of b
//     / tile_lo_fine [p]                                              pre_done[p]
//   plan_rec[p], plan[p]            k_plan(b); the queue head by      k_integrate(b)                       k_plan(b+3) on X(b+3) behind int_done[p] of b
//                                   k_integrate(b)
//   ctr_dev[call parity]            upload_ctr on X(first batch),     scatter, fix of the call's batches   the upload two calls later waits ctr_rd[parity][]
//                                   the other stream waits ctr_ev                                          of both pre-pass streams, recorded at the call's end
//   ht_key, ht_slot, unit_key,      k_prepare / k_plan of b and b+1 concurrently, with atomics (unit_slot_acquire); k_integrate takes slots from plan_rec
//     counters[C_NUNITS...]
//   pool                            k_integrate only                                                       order of V
//
// int_done[p] and pre_done[p] are re-recorded by every user of the slot: a wait captures the record in front of it in host order,
// which is why each wait is issued before the batch's own record of the same event.  The scatter and the constants copy touch
// nothing of slot p but dstage[p]; moving them in front of the wait (constants in a ring of their own) was measured and is slower:
// the two chains then fall into step, scatter next to scatter (profiles/r07a_ab_early_scatter.txt).
//
// The main stream of the pipeline is the handle's OWN stream even when the caller has set another one (er_tsdf_set_stream): HIP
// multiplexes streams over GPU_MAX_HW_QUEUES hardware queues (4 unless the process asks for more), and streams that share a queue
// run in order.  own_stream and the two pre-pass streams are created back to back and get a queue each; a caller's stream comes
// from elsewhere and lands on one of theirs -- with 4 queues k_integrate then stood in line behind a whole pre-pass chain and the
// voxel stream idled 240 us between launches instead of 15 (profiles/r07a_timeline_queues.txt: 146 k frames/s against 188 k with 8
// queues).  The two are joined at both ends: own_stream waits for what the caller's stream held when er_tsdf_integrate_frames
// began, and the caller's stream waits for the last voxel pass before the handle uses it for the volume again (join_voxel).
int run_batch(er_tsdf_t h, int n, const uint16_t* depth_dev, const double* T, const er_warp* warp, int frame0) {
  const int p = (int)(h->batch_no % kDepth), a = (int)(h->batch_no % kAux);
  h->batch_no++;
  er_tsdf_s::TimelineRow* tl = nullptr;                     // (the vector only grows here: the pointer holds until the batch returns)
  if (h->tl_on) {
    h->tl_rows.push_back(er_tsdf_s::TimelineRow{h->batch_no - 1, p, a, n, {host_now_ms() - h->tl_host0, 0.0, 0.0}, {}});
    tl = &h->tl_rows.back();
  }
  // Slot p was last used by batch n-3.  The HOST only needs its pinned constants block back (the H2D copy of batch n-3, an
  // early event); the DEVICE buffers of the slot (scaled depth, masks, frame constants) are protected on the device: the
  // pre-pass stream waits for k_integrate of batch n-3 before it touches them.  The host therefore never blocks on a voxel
  // pass and runs up to three batches ahead (host-frame copies and pre-passes queue up behind the events).
  if (h->used[p]) ER_HIP_TRY(hipEventSynchronize(h->consts_done[p]));
  if (tl) tl->host_ms[1] = host_now_ms() - h->tl_host0;
  Staging* st = reinterpret_cast<Staging*>(h->pinned[p].get());
  for (int f = 0; f < n; f++) {
    const double* Tf = T + (size_t)f * 16;
    double Tinv[16];
    if (!er::mat4_inverse(Tf, Tinv)) return er::fail("frame %d: singular pose matrix", frame0 + f);
    for (int q = 0; q < 12; q++) {
      st->fx[f].mi[q] = (float)Tinv[q];                          // trans_inv.cast<float>(), TSDFVolume.cpp:59
      st->t12[f * 12 + q] = Tf[q];
    }
    st->fx[f].tx = (float)Tf[3];                                 // transformation.cast<float>()(r,3)
    st->fx[f].ty = (float)Tf[7];
    st->fx[f].tz = (float)Tf[11];
    st->fx[f].pad = 0.f;
    for (int q = 0; q < 16; q++) st->fxT[q][f] = reinterpret_cast<const float*>(&st->fx[f])[q];
  }
  static_assert(offsetof(Staging, fxT) == sizeof(er::FrameXform) * ER_MAX_BATCH && sizeof(er::FrameXform) == 64, "fxT lies directly behind fx");
  hipStream_t X = h->aux_stream[a], S = h->own_stream;     // (the voxel stream: joined to h->stream by er_tsdf_integrate_frames)
  int* nbatch = h->counters + kNbatchSlot[p];

  constexpr int kIntBlocksPerCu = 3;                          // persistent workgroups fed by the queue.  Fewer than fit: the pre-pass kernels need register
                                           // space next to them (2 -> 172.0 k, 3 -> 174.3 k, 4 -> 170.0 k, 5 -> 169.6 k frames/s, profiles/r05n_*)
  const int wide_grid = h->n_cu * kIntBlocksPerCu;
  uint32_t* zsrc = nullptr;
  char* dst = static_cast<char*>(h->dstage[p]);
  const double* dev_t12 = reinterpret_cast<const double*>(dst + offsetof(Staging, t12));
  const double* dev_seg = reinterpret_cast<const double*>(dst + offsetof(Staging, seg));
  const double* dev_madj = reinterpret_cast<const double*>(dst + offsetof(Staging, madj));
  const int* dev_gi = reinterpret_cast<const int*>(dst + offsetof(Staging, gi));
  if (warp) {
    for (int f = 0; f < n; f++) {
      for (int q = 0; q < 12; q++) {
        st->seg[f * 16 + q] = warp->seg[(size_t)(frame0 + f) * 16 + q];
        st->madj[f * 12 + q] = warp->madj[(size_t)(frame0 + f) * 16 + q];
      }
      er::cube_coord_deltas(&st->seg[f * 16], h->cam, h->cols, h->rows, &st->seg[f * 16 + 12]);
      st->seg[f * 16 + 15] = 0.0;
      const int g = warp->grid_index[frame0 + f];
      if (g < 0 || g >= warp->num_grids) return er::fail("frame %d: control grid index %d out of [0,%d)", frame0 + f, g, warp->num_grids);
      st->gi[f] = g;
    }
  }
  // all per-batch constants travel in ONE copy kernel (every launch on this stream costs ~5 us of the pre-pass chain)
  if (h->used[p]) ER_HIP_TRY(hipStreamWaitEvent(X, h->int_done[p], 0));     // k_integrate of batch n-3 still reads dstage[p] / scaled[p] / plan_rec[p]
  if (tl && tl_record(h, &tl->ev[0], X)) return 1;
  static_assert(sizeof(Staging) % 4 == 0, "fetch_pinned copies 4-byte words");
  if (fetch_pinned(h->dstage[p], st, sizeof(Staging), X)) return 1;
  ER_HIP_TRY(hipEventRecord(h->consts_done[p], X));
  if (tl && tl_record(h, &tl->ev[1], X)) return 1;
  uint32_t ztag = 0;
  if (warp) {
    // every cell of zbuf is empty under this batch's tag: what earlier batches left carries theirs
    if (next_ztag(h, a, h->zbuf[a], (size_t)ER_MAX_BATCH * (size_t)h->pixels, X, &ztag)) return 1;
    const int verts = (warp->resolution + 1) * (warp->resolution + 1) * (warp->resolution + 1);
    const float grid_ul = warp->length / (float)warp->resolution;       // ControlGrid.cpp:19
    const ReprojArgs RA{depth_dev, n, h->cols, h->rows, h->cam, h->cami, dev_seg, dev_madj, dev_gi, h->ctr, warp->resolution, grid_ul,
                        verts * 3, h->zbuf[a], h->lastzero[a], h->zfix[a], h->counters + kZeroFlagSlot[a], ztag};
    if (launch_reproject(h, RA, n, X)) return 1;
    zsrc = h->zbuf[a];
  }
  if (tl && tl_record(h, &tl->ev[2], X)) return 1;

  // wide accesses (16 bytes per array and thread, 8 for the 16-bit depth): every frame base must be a multiple of four elements -- cols % 4 == 0
  // gives that for the handle's own buffers -- and a caller's device depth, which may sit at any 2-byte boundary, 8-byte aligned (the warped
  // path reads the z-buffer instead)
  const bool wide = h->cols % 4 == 0 && (zsrc || reinterpret_cast<uintptr_t>(depth_dev) % 8 == 0);
  hipLaunchKernelGGL(wide ? k_prepare<true> : k_prepare<false>, dim3((h->cols + kTile - 1) / kTile, (h->rows + kTile - 1) / kTile, n), dim3(kPrepThreads), 0, X,
                     depth_dev, zsrc, n, h->cols, h->rows, h->cam, h->cami, h->lambda, dev_t12, h->scaled[p], h->ht_key, h->ht_slot,
                     h->ht_mask[p], h->ht_cap - 1, h->ht_shift, h->batch[p], nbatch, h->counters,
                     h->tile_max[p], h->tile_lo[p], h->tile_lo_fine[p], make_int2(h->shard_rank, h->shard_world), h->lastzero[a], h->zfix[a],
                     h->counters + kZeroFlagSlot[a], ztag);
  if (tl && tl_record(h, &tl->ev[3], X)) return 1;
  hipLaunchKernelGGL(k_plan, dim3(1), dim3(256), 0, X, h->batch[p], nbatch, h->ht_mask[p], h->ht_key, h->ht_slot, h->unit_key, h->max_units,
                     h->counters, h->plan_rec[p], h->plan[p], warp ? h->counters + kZeroFlagSlot[a] : (int*)nullptr, h->stats);
  ER_HIP_TRY(hipGetLastError());
  if (tl && tl_record(h, &tl->ev[4], X)) return 1;
  ER_HIP_TRY(hipEventRecord(h->pre_done[p], X));

  ER_HIP_TRY(hipStreamWaitEvent(S, h->pre_done[p], 0));
  if (tl && tl_record(h, &tl->ev[5], S)) return 1;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  const bool timed = h->prof_stride > 0 && (h->prof_tick++ % h->prof_stride) == 0;
  if (timed) {
    ER_HIP_TRY(hipEventCreate(&e0));
    ER_HIP_TRY(hipEventCreate(&e1));
    ER_HIP_TRY(hipEventRecord(e0, S));
  }
  const bool sure = h->cam.integration_trunc < 64.0f;                   // voxel_classify's bound on the scaled depth (false for NaN)
  hipLaunchKernelGGL(sure ? k_integrate<true> : k_integrate<false>, dim3(wide_grid), dim3(kBlock), 0, S, h->pool, h->plan_rec[p], h->plan[p],
                     h->frames[p], h->scaled[p], h->tile_max[p], h->tile_lo[p], h->tile_lo_fine[p], (h->cols + kTile - 1) / kTile, (h->rows + kTile - 1) / kTile,
                     h->cam, h->cols, h->rows);
  if (timed) {
    ER_HIP_TRY(hipEventRecord(e1, S));
    h->events.emplace_back(e0, e1);
  }
  ER_HIP_TRY(hipGetLastError());
  if (tl && tl_record(h, &tl->ev[6], S)) return 1;
  ER_HIP_TRY(hipEventRecord(h->int_done[p], S));
  h->used[p] = true;
  h->frames_done += n;
  if (tl) tl->host_ms[2] = host_now_ms() - h->tl_host0;
  return 0;
}

}  // namespace

static hipError_t aux_create(hipStream_t* s) {
  // (stream priorities for the pre-pass streams, lowest or highest against the voxel stream's default: no effect on the job or on
  //  k_integrate's time in the pipeline, profiles/r03r_ab_stream_priority.txt)
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

extern "C" {

int er_tsdf_create(int cols, int rows, const float cam6[6], int max_units, int device, er_tsdf_t* out) {
  if (!out) return er::fail("er_tsdf_create: out is NULL");
  *out = nullptr;
  if (cols <= 0 || rows <= 0 || max_units <= 0) return er::fail("er_tsdf_create: bad dimensions");
  if ((long)cols * rows >= (1L << 30)) return er::fail("er_tsdf_create: image of %d x %d pixels is too large", cols, rows);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_tsdf_create: no HIP device available (liber_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return er::fail("er_tsdf_create: device %d out of range [0,%d)", device, ndev);
  ER_HIP_TRY(hipSetDevice(device));
  er_tsdf_t h = new er_tsdf_s();
  h->device = device;
  h->cols = cols;
  h->rows = rows;
  h->pixels = cols * rows;
  h->max_units = max_units;
  if (cam6) {
    h->cam = er::Camera{cam6[0], cam6[1], cam6[2], cam6[3], cam6[4], cam6[5]};
  } else {
    h->cam = er::Camera{525.0f, 525.0f, 319.5f, 239.5f, 2.5f, 2.5f};   // TSDFVolumeUnit.h:69
  }
  h->cami.inv_fx = 1.0 / (double)h->cam.fx;
  h->cami.inv_fy = 1.0 / (double)h->cam.fy;
  h->cami.pp_small = (std::fabs((double)h->cam.cx) < 1e6 && std::fabs((double)h->cam.cy) < 1e6) ? 1 : 0;
  h->cami.pad = 0;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cu = prop.multiProcessorCount;
  int cap = 1024, lg = 10;
  while (cap < 4 * max_units) { cap <<= 1; lg++; }
  h->ht_cap = cap;
  h->ht_shift = 32 - lg;
  const size_t px = (size_t)h->pixels, B = ER_MAX_BATCH;
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess ||
      aux_create(&h->aux_stream[0]) != hipSuccess || (kAux > 1 && aux_create(&h->aux_stream[kAux - 1]) != hipSuccess) ||
      false) {
    delete h;
    return er::fail("er_tsdf_create: hipStreamCreate failed");
  }
  h->stream = h->own_stream;
  if (hipEventCreateWithFlags(&h->caller_ev, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->voxel_done, hipEventDisableTiming) != hipSuccess) {
    er_tsdf_destroy(h);
    return er::fail("er_tsdf_create: event allocation failed");
  }
  for (int q = 0; q < kDepth; q++) {
    if (hipEventCreateWithFlags(&h->pre_done[q], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->int_done[q], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->copy_done[q], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->consts_done[q], hipEventDisableTiming) != hipSuccess ||
        h->pinned[q].reserve(sizeof(Staging), "er_tsdf_create")) {
      er_tsdf_destroy(h);
      return er::fail("er_tsdf_create: event / pinned staging allocation failed");
    }
  }
  // the fixed allocations: a failure has er::fail's text, and er_tsdf_destroy frees what came before it
  const char* who = "er_tsdf_create";
  er::DevScope& M = h->fixed;
  const size_t tiles = B * (size_t)((cols + kTile - 1) / kTile) * ((rows + kTile - 1) / kTile);
  const size_t tiles_fine = B * (size_t)((cols + (1 << kLoShift) - 1) >> kLoShift) * ((rows + (1 << kLoShift) - 1) >> kLoShift);
  bool bad = false;
  bad = bad || M.alloc(&h->pool, (size_t)max_units * er::kUnitVox, who);
  bad = bad || M.alloc(&h->ht_key, (size_t)cap, who);
  bad = bad || M.alloc(&h->ht_slot, (size_t)cap, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->ht_mask[q], (size_t)cap, who);
  bad = bad || M.alloc(&h->unit_key, (size_t)max_units, who);
  bad = bad || M.alloc(&h->counters, C_COUNT, who);
  bad = bad || M.alloc(&h->stats, 4, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->batch[q], (size_t)cap, who);
  bad = bad || M.alloc(&h->lambda, px, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->scaled[q], B * (px + kScaledPad), who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->depth_stage[q], B * px, who);
  for (int q = 0; q < kAux; q++) bad = bad || M.alloc(&h->zbuf[q], B * px, who);
  for (int q = 0; q < kAux; q++) bad = bad || M.alloc(&h->lastzero[q], B * px, who);
  for (int q = 0; q < kAux; q++) bad = bad || M.alloc(&h->zfix[q], B * px, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->dstage[q], sizeof(Staging), who);   // device twin of the pinned staging block: ONE copy per batch
  bad = bad || M.alloc(&h->T12, B * 12, who);
  bad = bad || M.alloc(&h->seg12, B * 16, who);
  bad = bad || M.alloc(&h->madj12, B * 12, who);
  bad = bad || M.alloc(&h->grid_index, B, who);
  bad = bad || M.alloc(&h->dsum, 1, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->tile_max[q], tiles, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->tile_lo[q], tiles, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->tile_lo_fine[q], tiles_fine, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->plan_rec[q], (size_t)cap, who);
  for (int q = 0; q < kDepth; q++) bad = bad || M.alloc(&h->plan[q], 1, who);
  if (bad) {
    er_tsdf_destroy(h);
    return 1;
  }
  for (int q = 0; q < kDepth; q++) h->frames[q] = reinterpret_cast<er::FrameXform*>(reinterpret_cast<char*>(h->dstage[q]) + offsetof(Staging, fx));
  hipStream_t s = h->stream;
  bool ok = hipMemsetAsync(h->pool, 0, (size_t)max_units * er::kUnitVox * sizeof(float2), s) == hipSuccess &&
            hipMemsetAsync(h->ht_key, 0xFF, (size_t)cap * sizeof(int), s) == hipSuccess &&
            hipMemsetAsync(h->ht_slot, 0xFF, (size_t)cap * sizeof(int), s) == hipSuccess &&
            hipMemsetAsync(h->counters, 0, C_COUNT * sizeof(int), s) == hipSuccess &&
            hipMemsetAsync(h->stats, 0, 4 * sizeof(unsigned long long), s) == hipSuccess;
  for (int q = 0; q < kDepth; q++)
    ok = ok && hipMemsetAsync(h->ht_mask[q], 0, (size_t)cap * sizeof(unsigned long long), s) == hipSuccess &&
         hipMemsetAsync(h->scaled[q], 0, B * (px + kScaledPad) * sizeof(float), s) == hipSuccess;   // (the pads stay zero)
  for (int q = 0; q < kAux; q++)
    ok = ok && hipMemsetAsync(h->lastzero[q], 0, B * px * sizeof(uint32_t), s) == hipSuccess &&
         hipMemsetAsync(h->zbuf[q], 0xFF, B * px * sizeof(uint32_t), s) == hipSuccess &&
         hipMemsetAsync(h->zfix[q], 0xFF, B * px * sizeof(uint32_t), s) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_lambda, dim3((h->pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, s, h->lambda, cols, rows, h->cam);
    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  if (!ok) {
    er_tsdf_destroy(h);
    return er::fail("er_tsdf_create: device initialisation failed: %s", hipGetErrorString(hipGetLastError()));
  }
  *out = h;
  return 0;
}

int er_tsdf_destroy(er_tsdf_t h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->own_stream && h->own_stream != h->stream) (void)hipStreamSynchronize(h->own_stream);
  if (h->caller_ev) (void)hipEventDestroy(h->caller_ev);
  if (h->voxel_done) (void)hipEventDestroy(h->voxel_done);
  for (auto& ev : h->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  for (int a = 0; a < kAux; a++)
    if (h->aux_stream[a]) (void)hipStreamSynchronize(h->aux_stream[a]);
  for (auto& r : h->tl_rows)
    for (hipEvent_t e : r.ev)
      if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->tl_free) (void)hipEventDestroy(e);
  if (h->tl_base) (void)hipEventDestroy(h->tl_base);
  for (int q = 0; q < kDepth; q++) {
    if (h->pre_done[q]) (void)hipEventDestroy(h->pre_done[q]);
    if (h->int_done[q]) (void)hipEventDestroy(h->int_done[q]);
    if (h->copy_done[q]) (void)hipEventDestroy(h->copy_done[q]);
    if (h->consts_done[q]) (void)hipEventDestroy(h->consts_done[q]);
    h->pinned[q].reset();
  }
  for (int a = 0; a < kAux; a++)
    if (h->aux_stream[a]) (void)hipStreamDestroy(h->aux_stream[a]);
  if (h->copy_stream) {
    (void)hipStreamSynchronize(h->copy_stream);
    (void)hipStreamDestroy(h->copy_stream);
  }
  for (int q = 0; q < 2; q++) {
    if (h->ctr_ev[q]) (void)hipEventDestroy(h->ctr_ev[q]);
    for (int a = 0; a < kAux; a++)
      if (h->ctr_rd[q][a]) (void)hipEventDestroy(h->ctr_rd[q][a]);
    h->ctr_pinned[q].reset();
  }
  static_cast<er_tsdf_mem&>(*h) = er_tsdf_mem();
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return 0;
}

int er_tsdf_set_stream(er_tsdf_t h, void* hip_stream) {
  if (!h) return er::fail("er_tsdf_set_stream: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (sync_all(h)) return 1;
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return 0;
}

int er_tsdf_synchronize(er_tsdf_t h) {
  if (!h) return er::fail("er_tsdf_synchronize: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  return sync_all(h);
}

int er_tsdf_scale_depth(er_tsdf_t h, const uint16_t* depth_host, float* scaled_host) {
  if (!h || !depth_host || !scaled_host) return er::fail("er_tsdf_scale_depth: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (sync_all(h)) return 1;
  const size_t px = (size_t)h->pixels;
  ER_HIP_TRY(hipMemcpyAsync(h->depth_stage[0], depth_host, px * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_scale_depth, dim3((h->pixels + kBlock - 1) / kBlock), dim3(kBlock), 0, h->stream, h->depth_stage[0],
                     h->lambda, h->scaled[0], h->pixels, h->cam.integration_trunc);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemcpyAsync(scaled_host, h->scaled[0], px * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

// num_grids lattices of (res+1)^3 x 3 floats -> device.
// The copy runs on the pre-pass stream of the call's first batch into the device buffer of this call's parity (so it never
// waits for the previous call's pre-passes, which read the other buffer); the other pre-pass stream (and `also`, if given)
// waits for it.  Sets h->ctr to the buffer the kernels of this call read.
static int upload_ctr(er_tsdf_t h, const float* ctr, int res, int num_grids, hipStream_t also) {
  const size_t verts = (size_t)(res + 1) * (res + 1) * (res + 1);
  const size_t floats = verts * 3 * (size_t)num_grids;
  const int q = h->ctr_parity;
  h->ctr_parity ^= 1;
  if (floats > h->ctr_dev[q].capacity()) {
    if (sync_all(h)) return 1;                       // nobody may still be reading the old buffer
    if (h->ctr_dev[q].reserve(floats, "er_tsdf_integrate_frames")) return 1;
  }
  // The lattices travel through a page-locked block of the handle: the copy is then truly asynchronous (a copy from the
  // caller's pageable memory would make the host wait for everything queued on this stream at every call) and the caller's
  // memory is free again when the call returns.
  if (!h->ctr_ev[q]) {
    ER_HIP_TRY(hipEventCreateWithFlags(&h->ctr_ev[q], hipEventDisableTiming));
    for (int a = 0; a < kAux; a++) ER_HIP_TRY(hipEventCreateWithFlags(&h->ctr_rd[q][a], hipEventDisableTiming));
  } else {
    ER_HIP_TRY(hipEventSynchronize(h->ctr_ev[q]));          // the upload of two calls ago (pinned block free again)
  }
  if (floats > h->ctr_pinned[q].capacity() && h->ctr_pinned[q].reserve(floats, "er_tsdf_integrate_frames")) return 1;
  memcpy(h->ctr_pinned[q], ctr, floats * sizeof(float));
  const int a0 = (int)(h->batch_no % kAux);
  hipStream_t C = h->aux_stream[a0];
  if (h->ctr_rd_set[q])                                     // the pre-passes of two calls ago read this device buffer
    for (int a = 0; a < kAux; a++)
      if (a != a0) ER_HIP_TRY(hipStreamWaitEvent(C, h->ctr_rd[q][a], 0));
  if (fetch_pinned(h->ctr_dev[q], h->ctr_pinned[q], floats * sizeof(float), C)) return 1;
  ER_HIP_TRY(hipEventRecord(h->ctr_ev[q], C));
  for (int a = 0; a < kAux; a++)
    if (a != a0) ER_HIP_TRY(hipStreamWaitEvent(h->aux_stream[a], h->ctr_ev[q], 0));
  if (also) ER_HIP_TRY(hipStreamWaitEvent(also, h->ctr_ev[q], 0));
  h->ctr = h->ctr_dev[q];
  h->ctr_cur = q;
  return 0;
}

// Reproject of n frames into zbuf: the all-exact kernel, or (-DER_REPROJECT_TIERED) tier 1 + the exact tail; then the replay launch.
static int launch_reproject(er_tsdf_t h, const ReprojArgs& RA, int n, hipStream_t X) {
  // (staging the lattice in LDS for this kernel was measured: slower, profiles/r02d_ab_lds_lattice.txt; a float32 tier with a
  //  per-pixel proof in front of the exact chain, four designs: slower, profiles/r02b / r02c / r02z_ab_tiered_reproject_*.txt)
  hipLaunchKernelGGL(k_reproject_scatter, dim3((h->cols + 63) / 64, (h->rows + 3) / 4, n), dim3(kBlock), 0, X, RA);
  hipLaunchKernelGGL(k_reproject_fix, dim3(kFixBlocks), dim3(kFixThreads), 0, X, RA);   // single waves: they have to find room next to three busy kernels
  ER_HIP_TRY(hipGetLastError());
  return 0;
}

int er_tsdf_reproject(er_tsdf_t h, uint16_t* depth_inout_host, const float* ctr_host, int resolution, float length,
                      const double seg[16], const double madj[16]) {
  if (!h || !depth_inout_host || !ctr_host || !seg || !madj) return er::fail("er_tsdf_reproject: NULL argument");
  if (resolution <= 0) return er::fail("er_tsdf_reproject: bad resolution");
  ER_HIP_TRY(hipSetDevice(h->device));
  const size_t px = (size_t)h->pixels;
  const int verts = (resolution + 1) * (resolution + 1) * (resolution + 1);
  if (sync_all(h)) return 1;                         // single-frame hook: runs alone on the main stream
  if (upload_ctr(h, ctr_host, resolution, 1, h->stream)) return 1;      // (on a pre-pass stream; the main stream waits for it)
  const int gi = 0;
  ER_HIP_TRY(hipMemcpyAsync(h->depth_stage[0], depth_inout_host, px * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
  double seg16[16] = {0};
  memcpy(seg16, seg, 12 * sizeof(double));
  er::cube_coord_deltas(seg16, h->cam, h->cols, h->rows, seg16 + 12);
  ER_HIP_TRY(hipMemcpyAsync(h->seg12, seg16, 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipMemcpyAsync(h->madj12, madj, 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  ER_HIP_TRY(hipMemcpyAsync(h->grid_index, &gi, sizeof(int), hipMemcpyHostToDevice, h->stream));
  const float grid_ul = length / (float)resolution;
  const long total = (long)px;
  uint32_t ztag = 0;                                   // (every stream is idle: the fill of a wrapping counter may run on this one)
  if (next_ztag(h, 0, h->zbuf[0], (size_t)ER_MAX_BATCH * px, h->stream, &ztag)) return 1;
  const ReprojArgs RA{h->depth_stage[0], 1, h->cols, h->rows, h->cam, h->cami, h->seg12, h->madj12, h->grid_index, h->ctr, resolution, grid_ul,
                      verts * 3, h->zbuf[0], h->lastzero[0], h->zfix[0], h->counters + kZeroFlagSlot[0], ztag};
  if (launch_reproject(h, RA, 1, h->stream)) return 1;
  hipLaunchKernelGGL(k_zbuf_to_depth, dim3((int)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, h->stream, h->zbuf[0],
                     h->depth_stage[0], total, h->lastzero[0], h->zfix[0], h->counters + kZeroFlagSlot[0], ztag);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemsetAsync(h->counters + kZeroFlagSlot[0], 0, 2 * sizeof(int), h->stream));
  ER_HIP_TRY(hipMemcpyAsync(depth_inout_host, h->depth_stage[0], px * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int er_tsdf_integrate_frames(er_tsdf_t h, int n, const uint16_t* depth, int depth_on_device, const double* T,
                             const er_warp* warp) {
  if (!h || !depth || !T) return er::fail("er_tsdf_integrate_frames: NULL argument");
  if (n < 0) return er::fail("er_tsdf_integrate_frames: negative frame count");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (n > 0) h->dropped.clear();                              // (handed-over units are zeroed: from here on they are this GPU's new contribution)
  if (warp) {
    if (!warp->ctr || !warp->grid_index || !warp->seg || !warp->madj || warp->num_grids <= 0 || warp->resolution <= 0)
      return er::fail("er_tsdf_integrate_frames: incomplete er_warp");
    if (upload_ctr(h, warp->ctr, warp->resolution, warp->num_grids, nullptr)) return 1;
  }
  const size_t px = (size_t)h->pixels;
  // n frames are fused in ceil(n / ER_MAX_BATCH) launches of (nearly) EQUAL size: 150 frames run as 3 x 50, not 64 + 64 + 22
  // (a voxel is loaded once per launch, so the short tail launch would pay the full volume traffic for a third of the frames)
  const int launches = (n + ER_MAX_BATCH - 1) / ER_MAX_BATCH;
  const int per = launches > 0 ? (n + launches - 1) / launches : 0;
  const bool joined = h->stream != h->own_stream && n > 0;    // the voxel passes run on own_stream (run_batch): behind the caller's stream ...
  if (joined) {
    ER_HIP_TRY(hipEventRecord(h->caller_ev, h->stream));
    ER_HIP_TRY(hipStreamWaitEvent(h->own_stream, h->caller_ev, 0));
  }
  for (int start = 0; start < n; start += per) {
    const int nb = std::min(per, n - start);
    const uint16_t* ddev;
    if (depth_on_device) {
      ddev = depth + (size_t)start * px;
    } else {
      // Host frames travel on their own stream into the staging buffer of this batch's slot: the copy of batch n+1 overlaps
      // the pre-passes of the batches before it (aux streams) and the voxel pass (main stream) when the caller's memory is
      // page-locked (er_host_alloc); pageable memory makes hipMemcpyAsync block the host, which is still correct.
      const int p = (int)(h->batch_no % kDepth);
      if (!h->copy_stream) ER_HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
      if (h->used[p]) ER_HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->pre_done[p], 0));   // the pre-pass that last read depth_stage[p] (batch n-3)
      ER_HIP_TRY(hipMemcpyAsync(h->depth_stage[p], depth + (size_t)start * px, (size_t)nb * px * sizeof(uint16_t),
                                hipMemcpyHostToDevice, h->copy_stream));
      ER_HIP_TRY(hipEventRecord(h->copy_done[p], h->copy_stream));
      ER_HIP_TRY(hipStreamWaitEvent(h->aux_stream[h->batch_no % kAux], h->copy_done[p], 0));
      ddev = h->depth_stage[p];
    }
    if (run_batch(h, nb, ddev, T + (size_t)start * 16, warp, start)) return 1;
  }
  // ... and in front of whatever the handle puts on the caller's stream next (join_voxel: own_stream is in order, so its last event will do)
  if (joined) {
    ER_HIP_TRY(hipEventRecord(h->voxel_done, h->own_stream));
    h->voxel_ahead = true;
  }
  if (warp) {                                              // the last readers of this call's lattice buffer, per pre-pass stream
    for (int a = 0; a < kAux; a++) ER_HIP_TRY(hipEventRecord(h->ctr_rd[h->ctr_cur][a], h->aux_stream[a]));
    h->ctr_rd_set[h->ctr_cur] = true;
  }
  // The caller may reuse or free its HOST frames as soon as the call returns: wait for the copies (not for the kernels).
  if (!depth_on_device && n > 0) ER_HIP_TRY(hipStreamSynchronize(h->copy_stream));
  return 0;
}

int er_tsdf_integrate(er_tsdf_t h, const uint16_t* depth_host, const double T[16]) {
  return er_tsdf_integrate_frames(h, 1, depth_host, 0, T, nullptr);
}

// Test hook (include/er_hip.h).  Nothing of the batch's pipeline slot that k_integrate read is overwritten before the slot's next batch: k_plan
// clears the hash map's frame masks and the list length, not plan_rec, which holds the {key, slot, mask} records, nor plan->n_units.
int er_tsdf_prepass_trace(er_tsdf_t h, int n, const uint16_t* depth, int depth_on_device, const double* T, const er_warp* warp,
                          float* scaled, int* scaled_pad, float* tile_max, float* tile_lo, float* tile_lo_fine,
                          int* keys, unsigned long long* masks, int keys_cap, int* n_keys) {
  if (!h) return er::fail("er_tsdf_prepass_trace: NULL handle");
  if (n < 1 || n > ER_MAX_BATCH) return er::fail("er_tsdf_prepass_trace: %d frames outside 1..%d (one batch)", n, ER_MAX_BATCH);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (sync_all(h)) return 1;
  const int p = (int)(h->batch_no % kDepth);
  if (er_tsdf_integrate_frames(h, n, depth, depth_on_device, T, warp)) return 1;
  if (sync_all(h)) return 1;
  const size_t B = ER_MAX_BATCH, px = (size_t)h->pixels;
  const size_t tiles = (size_t)((h->cols + kTile - 1) / kTile) * ((h->rows + kTile - 1) / kTile);
  const size_t fine = (size_t)((h->cols + (1 << kLoShift) - 1) >> kLoShift) * ((h->rows + (1 << kLoShift) - 1) >> kLoShift);
  if (scaled_pad) *scaled_pad = kScaledPad;
  if (scaled) ER_HIP_TRY(hipMemcpy(scaled, h->scaled[p], (size_t)n * (px + kScaledPad) * sizeof(float), hipMemcpyDeviceToHost));
  if (tile_max) ER_HIP_TRY(hipMemcpy(tile_max, h->tile_max[p], tiles * B * sizeof(float), hipMemcpyDeviceToHost));
  if (tile_lo) ER_HIP_TRY(hipMemcpy(tile_lo, h->tile_lo[p], tiles * B * sizeof(float), hipMemcpyDeviceToHost));
  if (tile_lo_fine) ER_HIP_TRY(hipMemcpy(tile_lo_fine, h->tile_lo_fine[p], fine * B * sizeof(float), hipMemcpyDeviceToHost));
  Plan plan{};
  ER_HIP_TRY(hipMemcpy(&plan, h->plan[p], sizeof plan, hipMemcpyDeviceToHost));
  if (plan.n_units < 0 || plan.n_units > h->ht_cap) return er::fail("er_tsdf_prepass_trace: the batch lists %d units", plan.n_units);
  if (n_keys) *n_keys = plan.n_units;
  if (keys || masks) {
    std::vector<PlanRec> rec((size_t)plan.n_units);
    if (plan.n_units > 0) ER_HIP_TRY(hipMemcpy(rec.data(), h->plan_rec[p], rec.size() * sizeof(PlanRec), hipMemcpyDeviceToHost));
    std::sort(rec.begin(), rec.end(), [](const PlanRec& a, const PlanRec& b) { return a.key < b.key; });
    for (int i = 0; i < plan.n_units && i < keys_cap; i++) {
      if (keys) keys[i] = rec[(size_t)i].key;
      if (masks) masks[i] = rec[(size_t)i].mask;
    }
  }
  return 0;
}

// Test hook (include/er_hip.h): the counter is only ever advanced, so that what earlier uses left in the buffer stays above the tags to come; a
// smaller value is reached through a fill, like a wrap.
int er_tsdf_set_zbuf_epoch(er_tsdf_t h, int which, unsigned epoch) {
  if (!h) return er::fail("er_tsdf_set_zbuf_epoch: NULL handle");
  if (which < 0 || which > kZColor) return er::fail("er_tsdf_set_zbuf_epoch: no z-buffer %d (0, 1: the pre-pass streams'; %d: the colour calls')", which, kZColor);
  if (epoch > kZEpochMax) return er::fail("er_tsdf_set_zbuf_epoch: epoch %u above %u", epoch, kZEpochMax);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (sync_all(h)) return 1;
  if (which < kAux && epoch < h->zepoch[which]) {            // (the colour calls fill their buffer at every call)
    ER_HIP_TRY(hipMemsetAsync(h->zbuf[which], 0xFF, (size_t)ER_MAX_BATCH * (size_t)h->pixels * sizeof(uint32_t), h->stream));
    ER_HIP_TRY(hipStreamSynchronize(h->stream));
  }
  h->zepoch[which] = epoch;
  return 0;
}

int er_tsdf_wait_event(er_tsdf_t h, void* hip_event) {
  if (!h || !hip_event) return er::fail("er_tsdf_wait_event: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  for (int a = 0; a < kAux; a++) ER_HIP_TRY(hipStreamWaitEvent(h->aux_stream[a], (hipEvent_t)hip_event, 0));
  if (h->copy_stream) ER_HIP_TRY(hipStreamWaitEvent(h->copy_stream, (hipEvent_t)hip_event, 0));
  return 0;
}

int er_tsdf_reset(er_tsdf_t h) {
  if (!h) return er::fail("er_tsdf_reset: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (sync_all(h)) return 1;
  int n = 0;
  ER_HIP_TRY(hipMemcpy(&n, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  n = std::min(std::max(n, 0), h->max_units);
  hipStream_t s = h->stream;
  if (n > 0) ER_HIP_TRY(hipMemsetAsync(h->pool, 0, (size_t)n * er::kUnitVox * sizeof(float2), s));   // only the units ever handed out
  if (n > 0 && h->color) ER_HIP_TRY(hipMemsetAsync(h->color, 0, (size_t)n * er::kUnitVox * 16, s));
  ER_HIP_TRY(hipMemsetAsync(h->ht_key, 0xFF, (size_t)h->ht_cap * sizeof(int), s));
  ER_HIP_TRY(hipMemsetAsync(h->ht_slot, 0xFF, (size_t)h->ht_cap * sizeof(int), s));
  for (int q = 0; q < kDepth; q++) ER_HIP_TRY(hipMemsetAsync(h->ht_mask[q], 0, (size_t)h->ht_cap * sizeof(unsigned long long), s));
  ER_HIP_TRY(hipMemsetAsync(h->counters, 0, C_COUNT * sizeof(int), s));
  for (int q = 0; q < kAux; q++) {
    ER_HIP_TRY(hipMemsetAsync(h->zbuf[q], 0xFF, (size_t)ER_MAX_BATCH * (size_t)h->pixels * sizeof(uint32_t), s));
    h->zepoch[q] = 0;
  }
  ER_HIP_TRY(hipStreamSynchronize(s));
  for (int q = 0; q < kDepth; q++) h->used[q] = false;
  h->batch_no = 0;
  h->dropped.clear();
  return 0;
}

int er_tsdf_set_unit_shard(er_tsdf_t h, int rank, int world) {
  if (!h) return er::fail("er_tsdf_set_unit_shard: NULL handle");
  if (world < 1 || rank < 0 || rank >= world) return er::fail("er_tsdf_set_unit_shard: rank %d not in [0,%d)", rank, world);
  ER_HIP_TRY(hipSetDevice(h->device));
  int n = 0;
  ER_HIP_TRY(hipMemcpy(&n, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  if (n != 0) return er::fail("er_tsdf_set_unit_shard: the volume already holds %d units (set the shard before the first frame)", n);
  h->shard_rank = rank;
  h->shard_world = world;
  return 0;
}

int er_unit_owner(int key, int world) { return er::unit_owner(key, world); }

int er_tsdf_status(er_tsdf_t h, int* flags, long* out_of_range_pixels) {
  if (!h) return er::fail("er_tsdf_status: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  int c[C_COUNT];
  ER_HIP_TRY(hipMemcpy(c, h->counters, sizeof c, hipMemcpyDeviceToHost));   // a poll: does not wait for the handle's (non-blocking) streams
  if (flags) *flags = (c[C_POOL_OVERFLOW] ? ER_STATUS_POOL_EXHAUSTED : 0) | (c[C_TABLE_FULL] ? ER_STATUS_TABLE_FULL : 0);
  if (out_of_range_pixels) *out_of_range_pixels = c[C_OUT_OF_RANGE];
  return 0;
}

int er_tsdf_unit_count(er_tsdf_t h, int* count) {
  if (!h || !count) return er::fail("er_tsdf_unit_count: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (check_flags(h)) return 1;
  ER_HIP_TRY(hipMemcpy(count, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  *count -= (int)h->dropped.size();                             // units handed to their owner by a distributed merge
  return 0;
}

int er_tsdf_unit_keys(er_tsdf_t h, int* keys_host) {
  if (!h || !keys_host) return er::fail("er_tsdf_unit_keys: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  std::vector<int> keys, slots;
  if (sorted_units(h, keys, slots)) return 1;
  std::copy(keys.begin(), keys.end(), keys_host);
  return 0;
}

int er_tsdf_read_unit(er_tsdf_t h, int key, float* sdf_host, float* weight_host) {
  if (!h) return er::fail("er_tsdf_read_unit: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (check_flags(h)) return 1;
  if (std::binary_search(h->dropped.begin(), h->dropped.end(), key)) return er::fail("er_tsdf_read_unit: unit %d was handed to its owner by the last merge", key);
  if (resolve_slots(h, &key, 1, false)) return 1;
  int slot = -1;
  ER_HIP_TRY(hipMemcpyAsync(&slot, h->slot_scratch, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (slot < 0) return er::fail("er_tsdf_read_unit: no unit with key %d", key);
  std::vector<float2> tmp((size_t)er::kUnitVox);
  ER_HIP_TRY(hipMemcpyAsync(tmp.data(), h->pool + (size_t)slot * er::kUnitVox, tmp.size() * sizeof(float2),
                            hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  for (int l = 0; l < er::kUnitVox; l++) {
    if (sdf_host) sdf_host[l] = tmp[(size_t)l].x;
    if (weight_host) weight_host[l] = tmp[(size_t)l].y;
  }
  return 0;
}

int er_tsdf_sum_weight(er_tsdf_t h, double* sum) {
  if (!h || !sum) return er::fail("er_tsdf_sum_weight: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (check_flags(h)) return 1;
  int n = 0;
  ER_HIP_TRY(hipMemcpy(&n, h->counters + C_NUNITS, sizeof(int), hipMemcpyDeviceToHost));
  ER_HIP_TRY(hipMemsetAsync(h->dsum, 0, sizeof(double), h->stream));
  if (n > 0) {
    hipLaunchKernelGGL(k_sum_weight, dim3(h->n_cu * 8), dim3(kBlock), 0, h->stream, h->pool, (long)n * er::kUnitVox, h->dsum);
    ER_HIP_TRY(hipGetLastError());
  }
  ER_HIP_TRY(hipMemcpyAsync(sum, h->dsum, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int er_tsdf_set_profiling(er_tsdf_t h, int enable) {
  if (!h) return er::fail("er_tsdf_set_profiling: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (join_voxel(h) || drain_events(h)) return 1;           // (behind every k_plan launched so far: their unit visits belong to the old account)
  h->prof_stride = enable > 0 ? enable : 0;
  h->prof_tick = 0;
  h->ms_total = 0.0;
  h->launches = 0;
  h->frames_done = 0;
  ER_HIP_TRY(hipMemsetAsync(h->stats, 0, 4 * sizeof(unsigned long long), h->stream));
  return 0;
}

int er_tsdf_get_profile(er_tsdf_t h, double* integrate_ms_total, long* integrate_launches, long* frames,
                        long* unit_visits) {
  if (!h) return er::fail("er_tsdf_get_profile: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  if (join_voxel(h)) return 1;                              // (the last voxel pass stands behind every k_plan, which account the unit visits)
  ER_HIP_TRY(hipStreamSynchronize(h->stream));
  if (drain_events(h)) return 1;
  unsigned long long st[4] = {0, 0, 0, 0};
  ER_HIP_TRY(hipMemcpy(st, h->stats, sizeof st, hipMemcpyDeviceToHost));
  if (integrate_ms_total) *integrate_ms_total = h->ms_total;
  if (integrate_launches) *integrate_launches = h->launches;
  if (frames) *frames = h->frames_done;
  if (unit_visits) *unit_visits = (long)st[0];
  return 0;
}

int er_tsdf_set_timeline(er_tsdf_t h, int on) {
  if (!h) return er::fail("er_tsdf_set_timeline: NULL handle");
  ER_HIP_TRY(hipSetDevice(h->device));
  h->tl_on = false;
  if (!on) return 0;                                         // (batches in flight keep their events; the rows stay readable)
  if (sync_all(h) || tl_drop_rows(h)) return 1;
  if (!h->tl_base) ER_HIP_TRY(hipEventCreate(&h->tl_base));
  ER_HIP_TRY(hipEventRecord(h->tl_base, h->own_stream));
  ER_HIP_TRY(hipEventSynchronize(h->tl_base));
  h->tl_host0 = host_now_ms();
  h->tl_on = true;
  return 0;
}

int er_tsdf_get_timeline(er_tsdf_t h, int cap, long long* meta, double* times_ms, int* n_rows) {
  if (!h || !n_rows) return er::fail("er_tsdf_get_timeline: NULL argument");
  ER_HIP_TRY(hipSetDevice(h->device));
  *n_rows = (int)h->tl_rows.size();
  if (!meta || !times_ms) return 0;
  if (cap < 0) return er::fail("er_tsdf_get_timeline: negative capacity");
  const int n = std::min(cap, *n_rows);
  *n_rows = 0;
  for (int i = 0; i < n; i++) {
    const er_tsdf_s::TimelineRow& r = h->tl_rows[(size_t)i];
    long long* m = meta + (size_t)i * ER_TIMELINE_META;
    double* t = times_ms + (size_t)i * ER_TIMELINE_TIMES;
    m[0] = r.batch;
    m[1] = r.slot;
    m[2] = r.stream;
    m[3] = r.frames;
    for (int q = 0; q < 3; q++) t[q] = r.host_ms[q];
    for (int q = 0; q < 7; q++) {
      float ms = -1.f;                                       // (a batch that failed half-way leaves the rest of its row unrecorded)
      if (r.ev[q]) {
        ER_HIP_TRY(hipEventSynchronize(r.ev[q]));
        ER_HIP_TRY(hipEventElapsedTime(&ms, h->tl_base, r.ev[q]));
      }
      t[3 + q] = (double)ms;
    }
  }
  if (tl_drop_rows(h)) return 1;
  *n_rows = n;
  return 0;
}

}  // extern "C"

namespace er_tsdf_k {

// er_tsdf_reproject's device part for the colour calls (er_tsdf_color.hip): frame 0 of RA through k_reproject_scatter and k_reproject_fix into
// RA.zbuf, then k_zbuf_to_depth into z_dev, which re-arms the two replay buffers; the flag words are cleared behind it.
int reproject_single(er_tsdf_t h, const ReprojArgs& RA, uint16_t* z_dev, hipStream_t X) {
  if (launch_reproject(h, RA, 1, X)) return 1;
  const long total = (long)RA.cols * RA.rows;
  hipLaunchKernelGGL(k_zbuf_to_depth, dim3((int)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, X, RA.zbuf, z_dev, total, RA.lastzero, RA.zfix,
                     RA.zero_flag, RA.ztag);
  ER_HIP_TRY(hipGetLastError());
  ER_HIP_TRY(hipMemsetAsync(RA.zero_flag, 0, 2 * sizeof(int), X));
  return 0;
}

}  // namespace er_tsdf_k
