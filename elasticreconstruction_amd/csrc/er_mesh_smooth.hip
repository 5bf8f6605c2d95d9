// er_mesh_smooth.hip -- Taubin lambda|mu smoothing of an indexed triangle mesh and vertex normals from its triangles, on the device (DESIGN.md
// 7.21; the definitions stand in include/er_hip.h above er_mesh_smooth, the per-element arithmetic in er_mesh_smooth_math.h).  A translation
// unit of its own: nothing here is compiled into the code object of any other file, and no other file's kernels are touched.
//
// Every result is defined without reference to an order of execution, and the kernels keep it that way with er_mesh_simplify.hip's discipline:
// no sort, no float atomic, and nothing is handed over inside a launch -- the launch boundary publishes.
//   - An edge is found through an open-addressing table of int32 slots that hold an INSTANCE INDEX 3 t + c; the key of a slot is the pair
//     (min, max) of the instance it holds, recomputed from the immutable triangles.  An instance claims an empty slot by compare-and-swap or,
//     where the slot's instance has its key, lowers the slot by atomicMin: which slot a key lands in depends on the order of arrival, the
//     minimum it ends up with -- the edge's representative -- does not.  A parallel array counts the instances of each slot: the multiplicity.
//   - The neighbours of a vertex are rows of a CSR built once per call: representatives count into deg, a three-launch scan on the device
//     turns deg into row starts (no host round trip), representatives fill the rows through per-row cursors.  The order inside a row depends
//     on arrival; no output does, because a row is only ever summed in int64.
//   - A pass is one thread per vertex over its row, reading one buffer and writing the other (Jacobi).
//   - The normals are 64-bit integer adds of each triangle's quantised cross product into its three vertices, then one thread per vertex.
#include "er_mesh.h"
#include "er_mesh_smooth_math.h"

#include <climits>
#include <cmath>

namespace {

using namespace er_tsdf_k;

constexpr int kSmBlock = 256;
constexpr unsigned long long kSmNone = ~0ull;
enum { W_EDGES = 0, W_BOUNDARY = 1, W_NONMANIFOLD = 2, W_STILL = 3, W_GUARD = 4, W_COUNT = 5 };   // the 64-bit words of a call
enum { D_PROBE = 0, D_FULL = 1, D_COUNT = 2 };                                                    // the diagnostic words

__device__ __forceinline__ int sm_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The first offending vertex and the first offending triangle, before any kernel uses an index as an address.  Lanes of a wave hold ascending
// indices: its lowest offending lane speaks for it.
__global__ __launch_bounds__(kSmBlock) void k_sm_check(const float4* __restrict__ verts, long nv, const int* __restrict__ tri, long nt,
                                                       unsigned long long* first) {
  const long i = (long)blockIdx.x * kSmBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool bad_v = false, bad_t = false;
  if (i < nv) {
    const float4 p = verts[i];
    bad_v = !er_sm::position_ok(p.x, p.y, p.z);
  }
  if (i < nt) {
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    bad_t = a < 0 || b < 0 || c < 0 || (long)a >= nv || (long)b >= nv || (long)c >= nv;
  }
  const unsigned long long bv = __ballot(bad_v), bt = __ballot(bad_t);
  if (bv && lane == __ffsll((long long)bv) - 1) atomicMin(first, (unsigned long long)i);
  if (bt && lane == __ffsll((long long)bt) - 1) atomicMin(first + 1, (unsigned long long)i);
}

// Instance i = 3 t + c: the pair tri[t][c], tri[t][(c + 1) % 3]; it is an edge iff the two differ.
struct SmEdge {
  int u, w;
  bool ok;
};

__device__ __forceinline__ SmEdge sm_edge(const int* __restrict__ tri, long i) {
  const long t = i / 3;
  const int c = (int)(i - 3 * t);
  SmEdge e;
  e.u = tri[i];
  e.w = tri[3 * t + (c == 2 ? 0 : c + 1)];
  e.ok = e.u != e.w;
  return e;
}

// One thread per instance: the edges into the table (size = mask + 1, a power of two, at least 2 ni, all -1).  slot[i] = where i's edge lives,
// mult[s] = the instances of slot s.  The largest probe count of the wave goes to diag[D_PROBE]; a sequence that ran through the whole
// table raises diag[D_FULL].
__global__ __launch_bounds__(kSmBlock) void k_sm_insert(const int* __restrict__ tri, long ni, int* table, unsigned long mask, unsigned* __restrict__ slot,
                                                        int* mult, int* diag) {
  const long i = (long)blockIdx.x * kSmBlock + threadIdx.x;
  bool active = i < ni;
  long probes = 0;
  bool placed = false;
  if (active) {
    const SmEdge me = sm_edge(tri, i);
    active = me.ok;
    if (me.ok) {
      const uint64_t key = er_sm::edge_key(me.u, me.w);
      unsigned long s = (unsigned long)er_sc::mix64(key) & mask;
      for (unsigned long n = 0; n <= mask; n++, s = (s + 1) & mask) {
        probes++;
        int cur = sm_load(table + s);
        if (cur < 0) {
          cur = atomicCAS(table + s, -1, (int)i);
          if (cur < 0) {
            placed = true;
            break;
          }
        }
        const SmEdge o = sm_edge(tri, cur);
        if (er_sm::edge_key(o.u, o.w) == key) {
          if (cur > (int)i) atomicMin(table + s, (int)i);
          placed = true;
          break;
        }
      }
      if (placed) {
        slot[i] = (unsigned)s;
        atomicAdd(mult + s, 1);
      }
    }
  }
  int p = active ? (int)(probes > (long)INT_MAX ? (long)INT_MAX : probes) : 0;
  for (int s = 32; s > 0; s >>= 1) p = max(p, __shfl_xor(p, s));
  if ((threadIdx.x & 63) == 0 && p > sm_load(diag + D_PROBE)) atomicMax(diag + D_PROBE, p);
  if (active && !placed) __hip_atomic_store(diag + D_FULL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Is instance i the representative of its edge?  (table and slot are final: the launch before published them.)
__device__ __forceinline__ bool sm_represents(const SmEdge& e, long i, const int* __restrict__ table, const unsigned* __restrict__ slot) {
  return e.ok && table[slot[i]] == (int)i;
}

// One thread per instance: the representative of each edge counts into the degrees of its two ends and marks them where its multiplicity is 1;
// words[W_EDGES ..] = distinct, boundary and non-manifold edges, one add per wave and word.
__global__ __launch_bounds__(kSmBlock) void k_sm_count(const int* __restrict__ tri, long ni, const int* __restrict__ table, const unsigned* __restrict__ slot,
                                                       const int* __restrict__ mult, int* deg, uint8_t* boundary, unsigned long long* words) {
  const long i = (long)blockIdx.x * kSmBlock + threadIdx.x;
  bool rep = false;
  int m = 0;
  if (i < ni) {
    const SmEdge e = sm_edge(tri, i);
    rep = sm_represents(e, i, table, slot);
    if (rep) {
      m = mult[slot[i]];
      atomicAdd(deg + e.u, 1);
      atomicAdd(deg + e.w, 1);
      if (m == 1) boundary[e.u] = boundary[e.w] = 1;           // (every writer writes the same byte)
    }
  }
  const unsigned long long b0 = __ballot(rep), b1 = __ballot(rep && m == 1), b2 = __ballot(rep && m >= 3);
  if ((threadIdx.x & 63) == 0) {
    if (b0) atomicAdd(words + W_EDGES, (unsigned long long)__popcll(b0));
    if (b1) atomicAdd(words + W_BOUNDARY, (unsigned long long)__popcll(b1));
    if (b2) atomicAdd(words + W_NONMANIFOLD, (unsigned long long)__popcll(b2));
  }
}

// x summed over lanes 0 .. lane of the wave
__device__ __forceinline__ unsigned sm_wave_scan(unsigned x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = __shfl_up(x, d);
    if (lane >= d) x += o;
  }
  return x;
}

// Every thread of the block comes with x: -> the sum of x over the threads below this one; *total = the block's sum.  One __syncthreads().
__device__ __forceinline__ unsigned sm_block_exclusive(unsigned x, unsigned (&lds)[kSmBlock / 64], unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned inc = sm_wave_scan(x, lane);
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < kSmBlock / 64; q++) {
    if (q < w) before += lds[q];
    all += lds[q];
  }
  *total = all;
  return before + inc - x;
}

// The scan of deg into row starts in three launches.  a: blk[b] = the degrees of block b; and the vertices that never move into words[W_STILL].
__global__ __launch_bounds__(kSmBlock) void k_sm_rows_a(const int* __restrict__ deg, const uint8_t* __restrict__ boundary, int fix, long nv,
                                                        unsigned* __restrict__ blk, unsigned long long* words) {
  __shared__ unsigned s_w[kSmBlock / 64];
  const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
  const unsigned d = v < nv ? (unsigned)deg[v] : 0u;
  const bool still = v < nv && (d == 0 || (fix && boundary[v] != 0));
  unsigned total;
  sm_block_exclusive(d, s_w, &total);
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
  const unsigned long long b = __ballot(still);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(words + W_STILL, (unsigned long long)__popcll(b));
}

// b: ONE block turns blk[0 .. nb) into its exclusive prefix, kSmBlock entries a round.
__global__ __launch_bounds__(kSmBlock) void k_sm_rows_b(unsigned* __restrict__ blk, long nb) {
  __shared__ unsigned s_w[kSmBlock / 64];
  unsigned carry = 0;
  for (long base = 0; base < nb; base += kSmBlock) {
    const long i = base + threadIdx.x;
    const unsigned x = i < nb ? blk[i] : 0u;
    unsigned total;
    const unsigned ex = sm_block_exclusive(x, s_w, &total);
    if (i < nb) blk[i] = carry + ex;
    carry += total;
    __syncthreads();                                           // (s_w is written again in the next round)
  }
}

// c: row[v] = the block's offset + the degrees of the block's vertices below v
__global__ __launch_bounds__(kSmBlock) void k_sm_rows_c(const int* __restrict__ deg, const unsigned* __restrict__ blk, long nv, unsigned* __restrict__ row) {
  __shared__ unsigned s_w[kSmBlock / 64];
  const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
  const unsigned d = v < nv ? (unsigned)deg[v] : 0u;
  unsigned total;
  const unsigned ex = sm_block_exclusive(d, s_w, &total);
  if (v < nv) row[v] = blk[blockIdx.x] + ex;
}

// One thread per instance: the representative of each edge writes either end into the row of the other, at the row's cursor.
__global__ __launch_bounds__(kSmBlock) void k_sm_fill(const int* __restrict__ tri, long ni, const int* __restrict__ table, const unsigned* __restrict__ slot,
                                                      const unsigned* __restrict__ row, int* cursor, int* __restrict__ adj) {
  const long i = (long)blockIdx.x * kSmBlock + threadIdx.x;
  if (i >= ni) return;
  const SmEdge e = sm_edge(tri, i);
  if (!sm_represents(e, i, table, slot)) return;
  adj[(unsigned long)row[e.u] + (unsigned long)atomicAdd(cursor + e.u, 1)] = e.w;
  adj[(unsigned long)row[e.w] + (unsigned long)atomicAdd(cursor + e.w, 1)] = e.u;
}

// One pass with factor f, one thread per vertex: dst = src moved towards the mean of its neighbours' quantised positions; a vertex without a
// neighbour, or one that still[] holds (nullable), keeps its bits.  run == 0 only copies (x y z 0).  A position that may not stand lowers
// *guard to pass << 32 | vertex.
__global__ __launch_bounds__(kSmBlock) void k_sm_pass(const float4* __restrict__ src, float4* __restrict__ dst, const unsigned* __restrict__ row,
                                                      const int* __restrict__ deg, const int* __restrict__ adj, const uint8_t* __restrict__ still, float f,
                                                      int run, long nv, unsigned pass, unsigned long long* guard) {
  const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool bad = false;
  if (v < nv) {
    const float4 p = src[v];
    float4 o = make_float4(p.x, p.y, p.z, 0.0f);
    const int d = run ? deg[v] : 0;
    if (d > 0 && !(still && still[v] != 0)) {
      const unsigned long r = row[v];
      long long S0 = 0, S1 = 0, S2 = 0;
      for (int j = 0; j < d; j++) {
        const float4 q = src[adj[r + (unsigned long)j]];
        S0 += er_sc::quantise(q.x);
        S1 += er_sc::quantise(q.y);
        S2 += er_sc::quantise(q.z);
      }
      o.x = er_sm::move(p.x, S0, d, f);
      o.y = er_sm::move(p.y, S1, d, f);
      o.z = er_sm::move(p.z, S2, d, f);
      bad = !er_sm::position_ok(o.x, o.y, o.z);
    }
    dst[v] = o;
  }
  const unsigned long long b = __ballot(bad);
  if (b && lane == __ffsll((long long)b) - 1) atomicMin(guard, (unsigned long long)pass << 32 | (unsigned long long)v);
}

// One thread per triangle: its quantised cross product into the sums of its three vertices (nsum[v] = N_x N_y N_z .), wrapping adds.
__global__ __launch_bounds__(kSmBlock) void k_sm_tri_normals(const float4* __restrict__ verts, const int* __restrict__ tri, long nt, unsigned long long* nsum) {
  const long t = (long)blockIdx.x * kSmBlock + threadIdx.x;
  if (t >= nt) return;
  const int i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
  const float4 A = verts[i[0]], B = verts[i[1]], C = verts[i[2]];
  const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
  long long k[3];
  er_sm::area_normal(a, b, c, k);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    if (k[q] == 0) continue;
#pragma unroll
    for (int n = 0; n < 3; n++) atomicAdd(nsum + 4 * (long)i[n] + q, (unsigned long long)k[q]);
  }
}

__global__ __launch_bounds__(kSmBlock) void k_sm_finish_normals(const unsigned long long* __restrict__ nsum, long nv, float4* __restrict__ nrm) {
  const long v = (long)blockIdx.x * kSmBlock + threadIdx.x;
  if (v >= nv) return;
  float g[3];
  er_sc::finish_normal((long long)nsum[4 * v], (long long)nsum[4 * v + 1], (long long)nsum[4 * v + 2], 1, g);
  nrm[v] = make_float4(g[0], g[1], g[2], 0.0f);
}

unsigned sm_grid(long n) { return (unsigned)((n + kSmBlock - 1) / kSmBlock); }

// slots of a table for n keys: a power of two, load at most 1/2
unsigned long sm_table_size(long n) {
  unsigned long size = 2;
  while (size < 2ul * (unsigned long)n) size <<= 1;
  return size;
}

// What the smoothing leaves in device memory: every array belongs to `owned` of the call; d_nrm is NULL when it was not asked for.
struct SmMesh {
  long stats[4] = {0, 0, 0, 0};
  long probes = 0;
  float4 *d_verts = nullptr, *d_nrm = nullptr;
  int* d_deg = nullptr;
  uint8_t* d_boundary = nullptr;
};

int sm_arguments(const char* who, int iterations, float lambda, float mu) {
  if (iterations < 0 || iterations > er_sm::kMaxIterations) return er::fail("%s: iterations = %d, outside [0, %d]", who, iterations, er_sm::kMaxIterations);
  if (!er_sm::factor_ok(lambda)) return er::fail("%s: lambda = %g; it has to be finite and at most 1 in magnitude", who, lambda);
  if (!er_sm::factor_ok(mu)) return er::fail("%s: mu = %g; it has to be finite and at most 1 in magnitude", who, mu);
  return 0;
}

// The smoothing of nv > 0 vertices and nt >= 0 triangles in device memory, on stream s, which it synchronises twice: for the first offenders of
// the input, and at the end for the guard word, the counts and the diagnostics.  Temporaries and results go to `owned`.
int smooth_on_device(const char* who, hipStream_t s, const float4* d_verts, long nv, const int* d_tri, long nt, int iterations, float lambda, float mu,
                     int fix_boundary, bool want_nrm, er::DevScope& owned, SmMesh* out) {
  // the first offenders
  unsigned long long *d_first = nullptr, *d_words = nullptr;
  int* d_diag = nullptr;
  if (owned.alloc(&d_first, 2, who)) return 1;
  if (owned.alloc(&d_words, W_COUNT, who)) return 1;
  if (owned.alloc(&d_diag, D_COUNT, who)) return 1;
  ER_W(who, hipMemsetAsync(d_first, 0xFF, 2 * sizeof(unsigned long long), s));
  ER_W(who, hipMemsetAsync(d_words, 0, W_COUNT * sizeof(unsigned long long), s));
  ER_W(who, hipMemsetAsync(d_words + W_GUARD, 0xFF, sizeof(unsigned long long), s));
  ER_W(who, hipMemsetAsync(d_diag, 0, D_COUNT * sizeof(int), s));
  hipLaunchKernelGGL(k_sm_check, dim3(sm_grid(std::max(nv, nt))), dim3(kSmBlock), 0, s, d_verts, nv, d_tri, nt, d_first);
  ER_W(who, hipGetLastError());
  unsigned long long first[2] = {kSmNone, kSmNone};
  ER_W(who, hipMemcpyAsync(first, d_first, sizeof first, hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  if (first[0] != kSmNone) {
    const long v = (long)first[0];
    float p[4] = {0, 0, 0, 0};
    ER_W(who, hipMemcpy(p, d_verts + v, sizeof p, hipMemcpyDeviceToHost));
    return er::fail("%s: vertex %ld (%g, %g, %g) has a coordinate that is not finite or not below 4096 m in magnitude", who, v, p[0], p[1], p[2]);
  }
  if (first[1] != kSmNone) {
    const long t = (long)first[1];
    int k[3] = {0, 0, 0};
    ER_W(who, hipMemcpy(k, d_tri + 3 * t, sizeof k, hipMemcpyDeviceToHost));
    for (int q = 0; q < 3; q++)
      if (k[q] < 0 || (long)k[q] >= nv) return er::fail("%s: triangle %ld names vertex %d, outside [0, %ld)", who, t, k[q], nv);
  }

  // edges, degrees, rows
  const long ni = 3 * nt, nbv = (long)sm_grid(nv), nbi = (long)sm_grid(ni);
  const unsigned long tsize = sm_table_size(ni);
  int *d_table = nullptr, *d_mult = nullptr, *d_deg = nullptr, *d_cursor = nullptr, *d_adj = nullptr;
  unsigned *d_slot = nullptr, *d_row = nullptr, *d_blk = nullptr;
  uint8_t* d_boundary = nullptr;
  float4* d_buf[2] = {nullptr, nullptr};
  if (owned.alloc(&d_deg, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_boundary, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_row, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_blk, (size_t)nbv, who)) return 1;
  if (owned.alloc(&d_buf[0], (size_t)nv, who)) return 1;
  ER_W(who, hipMemsetAsync(d_deg, 0, (size_t)nv * sizeof(int), s));
  ER_W(who, hipMemsetAsync(d_boundary, 0, (size_t)nv, s));
  if (nt > 0) {
    if (owned.alloc(&d_table, tsize, who)) return 1;
    if (owned.alloc(&d_mult, tsize, who)) return 1;
    if (owned.alloc(&d_slot, (size_t)ni, who)) return 1;
    if (owned.alloc(&d_cursor, (size_t)nv, who)) return 1;
    if (owned.alloc(&d_adj, (size_t)ni * 2, who)) return 1;    // (an edge has at least one instance: at most 2 ni entries)
    ER_W(who, hipMemsetAsync(d_table, 0xFF, tsize * sizeof(int), s));
    ER_W(who, hipMemsetAsync(d_mult, 0, tsize * sizeof(int), s));
    ER_W(who, hipMemsetAsync(d_slot, 0, (size_t)ni * sizeof(unsigned), s));   // (a slot that an overflowing table leaves unset is still an address)
    ER_W(who, hipMemsetAsync(d_cursor, 0, (size_t)nv * sizeof(int), s));
    hipLaunchKernelGGL(k_sm_insert, dim3((unsigned)nbi), dim3(kSmBlock), 0, s, d_tri, ni, d_table, tsize - 1, d_slot, d_mult, d_diag);
    hipLaunchKernelGGL(k_sm_count, dim3((unsigned)nbi), dim3(kSmBlock), 0, s, d_tri, ni, d_table, d_slot, d_mult, d_deg, d_boundary, d_words);
  }
  hipLaunchKernelGGL(k_sm_rows_a, dim3((unsigned)nbv), dim3(kSmBlock), 0, s, d_deg, d_boundary, fix_boundary ? 1 : 0, nv, d_blk, d_words);
  hipLaunchKernelGGL(k_sm_rows_b, dim3(1), dim3(kSmBlock), 0, s, d_blk, nbv);
  hipLaunchKernelGGL(k_sm_rows_c, dim3((unsigned)nbv), dim3(kSmBlock), 0, s, d_deg, d_blk, nv, d_row);
  if (nt > 0) hipLaunchKernelGGL(k_sm_fill, dim3((unsigned)nbi), dim3(kSmBlock), 0, s, d_tri, ni, d_table, d_slot, d_row, d_cursor, d_adj);
  ER_W(who, hipGetLastError());

  // the passes: pass 2 i has the factor lambda, pass 2 i + 1 the factor mu; one whose factor is 0 is not run and keeps its number
  const float4* cur = d_verts;
  int ran = 0;
  for (int k = 0; k < 2 * iterations; k++) {
    const float f = (k & 1) ? mu : lambda;
    if (f == 0.0f) continue;
    if (ran == 1 && owned.alloc(&d_buf[1], (size_t)nv, who)) return 1;
    float4* dst = d_buf[ran & 1];
    hipLaunchKernelGGL(k_sm_pass, dim3((unsigned)nbv), dim3(kSmBlock), 0, s, cur, dst, d_row, d_deg, d_adj, fix_boundary ? d_boundary : nullptr, f, 1, nv,
                       (unsigned)k, d_words + W_GUARD);
    cur = dst;
    ran++;
  }
  if (!ran) {                                                  // the input's bits with the 4th column 0
    hipLaunchKernelGGL(k_sm_pass, dim3((unsigned)nbv), dim3(kSmBlock), 0, s, cur, d_buf[0], d_row, d_deg, d_adj, nullptr, 0.0f, 0, nv, 0u, d_words + W_GUARD);
    cur = d_buf[0];
  }
  ER_W(who, hipGetLastError());

  // the normals of the triangles at the positions the passes left
  float4* d_nrm = nullptr;
  if (want_nrm) {
    unsigned long long* d_nsum = nullptr;
    if (owned.alloc(&d_nsum, (size_t)nv * 4, who)) return 1;
    if (owned.alloc(&d_nrm, (size_t)nv, who)) return 1;
    ER_W(who, hipMemsetAsync(d_nsum, 0, (size_t)nv * 4 * sizeof(unsigned long long), s));
    if (nt > 0) hipLaunchKernelGGL(k_sm_tri_normals, dim3(sm_grid(nt)), dim3(kSmBlock), 0, s, cur, d_tri, nt, d_nsum);
    hipLaunchKernelGGL(k_sm_finish_normals, dim3((unsigned)nbv), dim3(kSmBlock), 0, s, d_nsum, nv, d_nrm);
    ER_W(who, hipGetLastError());
  }

  // the end: the guard word, the counts, the diagnostics
  unsigned long long words[W_COUNT] = {0, 0, 0, 0, kSmNone};
  int diag[D_COUNT] = {0, 0};
  ER_W(who, hipMemcpyAsync(words, d_words, sizeof words, hipMemcpyDeviceToHost, s));
  ER_W(who, hipMemcpyAsync(diag, d_diag, sizeof diag, hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  if (diag[D_FULL]) return er::fail("%s: a probe sequence ran through its whole table (%lu slots)", who, tsize);
  if (words[W_GUARD] != kSmNone) {
    const long pass = (long)(words[W_GUARD] >> 32), v = (long)(words[W_GUARD] & 0xFFFFFFFFull);
    return er::fail("%s: pass %ld (iteration %ld, %s) moves vertex %ld to a coordinate that is not finite or not below 4096 m in magnitude", who, pass,
                    pass / 2, (pass & 1) ? "mu" : "lambda", v);
  }
  for (int q = 0; q < 4; q++) out->stats[q] = (long)words[q];
  out->probes = diag[D_PROBE];
  out->d_verts = const_cast<float4*>(cur);
  out->d_nrm = d_nrm;
  out->d_deg = d_deg;
  out->d_boundary = d_boundary;
  return 0;
}

}  // namespace

extern "C" {

int er_mesh_smooth(const float* verts_host, long n_vertices, const int* tri_host, long n_triangles, int iterations, float lambda, float mu,
                   int fix_boundary, int device, float* verts_out, float* normals_out, int* degree_out, uint8_t* boundary_out, long stats[4],
                   long probes[1]) {
  const char* who = "er_mesh_smooth";
  if ((n_vertices > 0 && !verts_host) || (n_triangles > 0 && !tri_host)) return er::fail("er_mesh_smooth: NULL argument");
  if (n_triangles < 0 || n_vertices < 0) return er::fail("er_mesh_smooth: %ld triangles, %ld vertices", n_triangles, n_vertices);
  if (n_vertices > (long)INT_MAX) return er::fail("er_mesh_smooth: %ld vertices; the limit is 2^31 - 1 (int32 indices)", n_vertices);
  if (n_triangles > (long)INT_MAX / 3) return er::fail("er_mesh_smooth: %ld triangles; the limit is 3 * triangles <= 2^31 - 1 (int32 edge instances)", n_triangles);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return er::fail("er_mesh_smooth: no HIP device available (liber_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return er::fail("er_mesh_smooth: device %d of %d", device, ndev);
  if (sm_arguments(who, iterations, lambda, mu)) return 1;
  const long nv = n_vertices, nt = n_triangles;
  if (nv == 0) {                                               // nothing to smooth: no triangle is looked at
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (probes) probes[0] = 0;
    return 0;
  }
  ER_HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;                                     // (the null stream: the call is synchronous)
  er::DevScope own;
  float4* d_verts = nullptr;
  int* d_tri = nullptr;
  if (own.alloc(&d_verts, (size_t)nv, who)) return 1;
  if (own.alloc(&d_tri, (size_t)nt * 3, who)) return 1;
  ER_W(who, hipMemcpyAsync(d_verts, verts_host, (size_t)nv * sizeof(float4), hipMemcpyHostToDevice, s));
  if (nt > 0) ER_W(who, hipMemcpyAsync(d_tri, tri_host, (size_t)nt * 3 * sizeof(int), hipMemcpyHostToDevice, s));
  SmMesh r;
  if (smooth_on_device(who, s, d_verts, nv, d_tri, nt, iterations, lambda, mu, fix_boundary, normals_out != nullptr, own, &r)) return 1;
  for (int q = 0; q < 4 && stats; q++) stats[q] = r.stats[q];
  if (probes) probes[0] = r.probes;
  if (verts_out) ER_W(who, hipMemcpyAsync(verts_out, r.d_verts, (size_t)nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (normals_out) ER_W(who, hipMemcpyAsync(normals_out, r.d_nrm, (size_t)nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (degree_out) ER_W(who, hipMemcpyAsync(degree_out, r.d_deg, (size_t)nv * sizeof(int), hipMemcpyDeviceToHost, s));
  if (boundary_out) ER_W(who, hipMemcpyAsync(boundary_out, r.d_boundary, (size_t)nv, hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  return 0;
}

int er_tsdf_extract_mesh_smoothed(er_tsdf_t h, int iterations, float lambda, float mu, int fix_boundary, float cell, long min_triangles,
                                  int largest_only, int want_colors, float* verts_host, float* normals_host, uint8_t* colors_host,
                                  long capacity_vertices, int* tri_host, long capacity_triangles, long* n_vertices, long* n_triangles,
                                  long smooth_stats[4], long simplify_stats[4], long before[2]) {
  const char* who = "er_tsdf_extract_mesh_smoothed";
  if (!h || !n_vertices || !n_triangles) return er::fail("er_tsdf_extract_mesh_smoothed: NULL argument");
  if (min_triangles < 0) return er::fail("er_tsdf_extract_mesh_smoothed: min_triangles = %ld", min_triangles);
  if (colors_host && !want_colors) return er::fail("er_tsdf_extract_mesh_smoothed: an output of colours without want_colors");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_tsdf_extract_mesh_smoothed: no HIP device available (liber_hip has no CPU fallback)");
  if (sm_arguments(who, iterations, lambda, mu)) return 1;
  if (!(std::isfinite(cell) && cell >= 0.0f)) return er::fail("er_tsdf_extract_mesh_smoothed: cell = %g m; it has to be finite and not below 0", cell);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (want_colors && color_sample_on_device(h, who, nullptr, 0, nullptr)) return 1;
  *n_vertices = *n_triangles = 0;
  for (int q = 0; q < 4; q++) {
    if (smooth_stats) smooth_stats[q] = 0;
    if (simplify_stats) simplify_stats[q] = 0;
  }
  if (before) before[0] = before[1] = 0;
  hipStream_t s = h->stream;
  const bool cluster = cell > 0.0f, smoothing = iterations > 0;
  const bool tsdf_normals = normals_host != nullptr && !smoothing;   // (a moved vertex has the normal of its triangles)
  const bool want_rows = verts_host || normals_host || colors_host;

  // Without the clustering the counts are those of the mesh that is smoothed: they are set, and the capacities refused, before any array is made.
  auto capacities = [&](long nv, long nt) {
    if (cluster) return 0;
    *n_vertices = nv;
    *n_triangles = nt;
    if (want_rows && capacity_vertices < nv) return er::fail("er_tsdf_extract_mesh_smoothed: capacity %ld < %ld vertices", capacity_vertices, nv);
    if (tri_host && capacity_triangles < nt) return er::fail("er_tsdf_extract_mesh_smoothed: capacity %ld < %ld triangles", capacity_triangles, nt);
    return 0;
  };

  // the mesh, cleaned where that is asked for: it stays in device memory
  ScMesh r;                                                    // (r and c before m: their lists outlive the copies that m's hipFree waits for)
  CleanedMesh c;
  DeviceMesh m;
  const float4 *d_verts = nullptr, *d_nrm = nullptr;
  const int* d_tri = nullptr;
  long nv = 0, nt = 0;
  if (min_triangles > 1 || largest_only) {
    auto counted = [&](const CleanedMesh& c) { return capacities(c.nv, c.ntri); };
    if (mesh_cleaned_on_device(h, who, min_triangles, largest_only, true, tsdf_normals, true, true, counted, &m, &c)) return 1;
    nv = c.nv;
    nt = c.ntri;
    d_verts = c.d_verts;
    d_nrm = c.d_nrm;
    d_tri = c.d_tri;
  } else {
    auto counted = [&](long n, long t) {
      if (n > (long)INT_MAX) return er::fail("er_tsdf_extract_mesh_smoothed: %ld vertices; the limit is 2^31 - 1 (int32 indices)", n);
      if (t > (long)INT_MAX / 3) return er::fail("er_tsdf_extract_mesh_smoothed: %ld triangles; the limit is 3 * triangles <= 2^31 - 1", t);
      return capacities(n, t);
    };
    if (mesh_indexed_on_device(h, who, true, tsdf_normals, true, &nv, &nt, counted, &m)) return 1;
    d_verts = m.d_verts;
    d_nrm = m.d_nrm;
    d_tri = m.d_tri;
  }
  if (nv == 0 || nt == 0 || !d_verts || !d_tri) {              // an empty volume, one without a crossing, or nothing left of it
    *n_vertices = *n_triangles = 0;
    return 0;
  }
  if (nt > (long)INT_MAX / 3) return er::fail("er_tsdf_extract_mesh_smoothed: %ld triangles; the limit is 3 * triangles <= 2^31 - 1", nt);
  if (before) {
    before[0] = nv;
    before[1] = nt;
  }
  if (!cluster && !want_rows && !tri_host && !smooth_stats) return 0;   // counts only: those of the mesh that would be smoothed
  uchar4* d_rgba = nullptr;
  if (colors_host) {                                           // the colours of the unsmoothed vertices, sampled where the surface was observed
    if (m.owned.alloc(&d_rgba, (size_t)nv, who)) return 1;
    if (color_sample_on_device(h, who, d_verts, nv, d_rgba)) return 1;
  }
  if (smoothing) {
    SmMesh sm;
    if (smooth_on_device(who, s, d_verts, nv, d_tri, nt, iterations, lambda, mu, fix_boundary, normals_host != nullptr, m.owned, &sm)) return 1;
    for (int q = 0; q < 4 && smooth_stats; q++) smooth_stats[q] = sm.stats[q];
    d_verts = sm.d_verts;
    d_nrm = sm.d_nrm;
  }
  if (!cluster) {
    if (verts_host) ER_W(who, hipMemcpyAsync(verts_host, d_verts, (size_t)nv * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (normals_host) ER_W(who, hipMemcpyAsync(normals_host, d_nrm, (size_t)nv * sizeof(float4), hipMemcpyDeviceToHost, s));
    if (colors_host) ER_W(who, hipMemcpyAsync(colors_host, d_rgba, (size_t)nv * sizeof(uchar4), hipMemcpyDeviceToHost, s));
    if (tri_host) ER_W(who, hipMemcpyAsync(tri_host, d_tri, (size_t)nt * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    ER_W(who, hipStreamSynchronize(s));
    return 0;
  }
  const ScWant want{verts_host != nullptr, normals_host != nullptr, colors_host != nullptr, false, tri_host != nullptr, false, false};
  auto counted = [&](const ScMesh& r) {
    *n_vertices = r.nv;
    *n_triangles = r.ntri;
    for (int q = 0; q < 4 && simplify_stats; q++) simplify_stats[q] = r.stats[q];
    if (want_rows && capacity_vertices < r.nv) return er::fail("er_tsdf_extract_mesh_smoothed: capacity %ld < %ld vertices", capacity_vertices, r.nv);
    if (want.tri && capacity_triangles < r.ntri) return er::fail("er_tsdf_extract_mesh_smoothed: capacity %ld < %ld triangles", capacity_triangles, r.ntri);
    return 0;
  };
  if (simplify_on_device(who, s, d_verts, d_nrm, d_rgba, nv, d_tri, nt, cell, want, counted, m.owned, &r)) return 1;
  return sc_copy_back(who, s, r, nv, verts_host, normals_host, colors_host, nullptr, tri_host, nullptr, nullptr);
}

}  // extern "C"
