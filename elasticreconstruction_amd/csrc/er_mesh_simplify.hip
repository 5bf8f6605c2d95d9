// er_mesh_simplify.hip -- vertex clustering (Rossignac-Borrel) of an indexed triangle mesh on the device (the definitions stand
// in include/er_hip.h above er_mesh_simplify, the per-element arithmetic in er_mesh_simplify_math.h).  A translation unit of its own: nothing
// here is compiled into the code object of any other file, and no other file's kernels are touched.
//
// Every result is defined without reference to an order of execution, and the kernels keep it that way with er_mesh_cc.hip's discipline:
// no sort, no float atomic, and nothing is handed over inside a launch -- the launch boundary publishes.
//   - A cluster is found through an open-addressing table of int32 slots that hold a VERTEX INDEX; the key of a slot is the key of the vertex it
//     holds, recomputed from the immutable input.  A vertex claims an empty slot by compare-and-swap or, where the slot's vertex has its key,
//     lowers the slot by atomicMin.  Once a slot is claimed only members of one cluster ever replace its value, so its key never changes: which
//     slot a key lands in depends on the order of arrival, the minimum it ends up with -- the cluster's lead -- does not.
//   - The sums of a cluster are 64-bit integer adds into the row of its lead: exact, associative.  Neighbouring vertices of an extracted mesh
//     mostly share a cell, so a wave first adds up its runs of equal lead (a segmented scan) and sends one add per run and word.
//   - Duplicate triangles meet in a second table of the same kind, keyed by the canonical rotation of the triple of leads and holding the
//     lowest TRIANGLE INDEX.
//   - Vertices and triangles are compacted in two passes with the host's prefix over the block counts between them (er_compact.h).
#include "er_mesh.h"
#include "er_mesh_simplify_math.h"

#include <climits>
#include <cmath>

namespace {

using namespace er_tsdf_k;

constexpr int kScBlock = 256;
constexpr unsigned long long kScNone = ~0ull;
enum { D_PROBE_V = 0, D_PROBE_T = 1, D_FULL = 2, D_COUNT = 4 };   // the diagnostic words

__device__ __forceinline__ int sc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint64_t sc_key(const float4* __restrict__ verts, long v, float cell) {
  const float4 p = verts[v];
  return er_sc::cell_key(p.x, p.y, p.z, cell);
}

// The first offending vertex and the first offending triangle, before any kernel uses an index as an address or a cell as a key.  Lanes of a
// wave hold ascending indices: its lowest offending lane speaks for it.
__global__ __launch_bounds__(kScBlock) void k_sc_check(const float4* __restrict__ verts, long nv, float cell, const int* __restrict__ tri, long nt,
                                                       unsigned long long* first) {
  const long i = (long)blockIdx.x * kScBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool bad_v = false, bad_t = false;
  if (i < nv) {
    const float4 p = verts[i];
    bad_v = er_sc::vertex_offence(p.x, p.y, p.z, cell) != 0;
  }
  if (i < nt) {
    const int a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
    bad_t = a < 0 || b < 0 || c < 0 || (long)a >= nv || (long)b >= nv || (long)c >= nv;
  }
  const unsigned long long bv = __ballot(bad_v), bt = __ballot(bad_t);
  if (bv && lane == __ffsll((long long)bv) - 1) atomicMin(first, (unsigned long long)i);
  if (bt && lane == __ffsll((long long)bt) - 1) atomicMin(first + 1, (unsigned long long)i);
}

// The largest probe count of the wave into diag[which]; more probes than the table has slots raise diag[D_FULL].
__device__ __forceinline__ void sc_report(long probes, bool placed, bool active, int* diag, int which) {
  int p = active ? (int)(probes > (long)INT_MAX ? (long)INT_MAX : probes) : 0;
  for (int s = 32; s > 0; s >>= 1) p = max(p, __shfl_xor(p, s));
  if ((threadIdx.x & 63) == 0 && p > sc_load(diag + which)) atomicMax(diag + which, p);
  if (active && !placed) __hip_atomic_store(diag + D_FULL, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One thread per vertex: into the table (size = mask + 1, a power of two, at least 2 nv, all -1).  slot[v] = where v's cluster lives.
__global__ __launch_bounds__(kScBlock) void k_sc_insert(const float4* __restrict__ verts, long nv, float cell, int* table, unsigned long mask,
                                                        unsigned* __restrict__ slot, int* diag) {
  const long v = (long)blockIdx.x * kScBlock + threadIdx.x;
  const bool active = v < nv;
  long probes = 0;
  bool placed = false;
  if (active) {
    const uint64_t key = sc_key(verts, v, cell);
    unsigned long s = (unsigned long)er_sc::mix64(key) & mask;
    for (unsigned long n = 0; n <= mask; n++, s = (s + 1) & mask) {
      probes++;
      int cur = sc_load(table + s);
      if (cur < 0) {
        cur = atomicCAS(table + s, -1, (int)v);
        if (cur < 0) {
          placed = true;
          break;
        }
      }
      if (sc_key(verts, cur, cell) == key) {
        if (cur > (int)v) atomicMin(table + s, (int)v);
        placed = true;
        break;
      }
    }
    if (placed) slot[v] = (unsigned)s;
  }
  sc_report(probes, placed, active, diag, D_PROBE_V);
}

// x summed over the lanes start .. lane of the wave
__device__ __forceinline__ long long sc_scan(long long x, int lane, int start) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(x, d);
    if (lane - d >= start) x += o;
  }
  return x;
}

__device__ __forceinline__ void sc_add(unsigned long long* p, long long x) {
  if (x != 0) atomicAdd(p, (unsigned long long)x);
}

// One thread per vertex: lead[v] = the minimum its slot ended up with, and the cluster's sums into the rows of the lead -- pos[L] = S_x S_y S_z n,
// nsum[L] = N_x N_y N_z contributors, csum[L] = r g b members with a != 0 (the last two where the arrays exist).  A run of lanes with one lead
// sends one add per word from its last lane.
__global__ __launch_bounds__(kScBlock) void k_sc_sums(const float4* __restrict__ verts, const float4* __restrict__ nrm, const uchar4* __restrict__ rgba,
                                                      long nv, const int* __restrict__ table, const unsigned* __restrict__ slot,
                                                      int* __restrict__ lead, unsigned long long* pos, unsigned long long* nsum,
                                                      unsigned long long* csum) {
  const long v = (long)blockIdx.x * kScBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = v < nv;
  const int L = active ? table[slot[v]] : -1;
  if (active) lead[v] = L;
  const int prev = __shfl_up(L, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != L);
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  const bool tail = active && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
  long long q[3] = {0, 0, 0};
  if (active) {
    const float4 p = verts[v];
    q[0] = er_sc::quantise(p.x);
    q[1] = er_sc::quantise(p.y);
    q[2] = er_sc::quantise(p.z);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const long long s = sc_scan(q[a], lane, start);
    if (tail) sc_add(pos + 4 * (long)L + a, s);
  }
  if (tail) sc_add(pos + 4 * (long)L + 3, (long long)(lane - start + 1));
  if (nrm) {                                                   // (uniform over the launch)
    long long g[4] = {0, 0, 0, 0};
    if (active) {
      const float4 n = nrm[v];
      if (er_sc::normal_contributes(n.x, n.y, n.z)) {
        g[0] = er_sc::quantise(n.x);
        g[1] = er_sc::quantise(n.y);
        g[2] = er_sc::quantise(n.z);
        g[3] = 1;
      }
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const long long s = sc_scan(g[a], lane, start);
      if (tail) sc_add(nsum + 4 * (long)L + a, s);
    }
  }
  if (rgba) {
    long long c = 0;                                           // r | g << 16 | b << 32 | count << 48: 64 lanes of at most 255 stay below 2^14 a field
    if (active) {
      const uchar4 k = rgba[v];
      if (k.w != 0) c = (long long)k.x | (long long)k.y << 16 | (long long)k.z << 32 | 1ll << 48;
    }
    const long long s = sc_scan(c, lane, start);
    if (tail) {
#pragma unroll
      for (int a = 0; a < 4; a++) sc_add(csum + 4 * (long)L + a, (s >> (16 * a)) & 0xFFFF);
    }
  }
}

struct ScTriple {
  int k[3];
  bool ok;                                                     // three different clusters
};

__device__ __forceinline__ ScTriple sc_triple(const int* __restrict__ tri, const int* __restrict__ lead, long t) {
  const int A = lead[tri[3 * t]], B = lead[tri[3 * t + 1]], C = lead[tri[3 * t + 2]];
  ScTriple r;
  r.ok = A != B && B != C && A != C;
  er_sc::canonical_rotation(A, B, C, r.k);
  return r;
}

// One thread per triangle: the non-degenerate ones into their table, which ends up holding the lowest triangle index of every canonical triple.
__global__ __launch_bounds__(kScBlock) void k_st_insert(const int* __restrict__ tri, long nt, const int* __restrict__ lead, int* table, unsigned long mask,
                                                        unsigned* __restrict__ slot, int* diag) {
  const long t = (long)blockIdx.x * kScBlock + threadIdx.x;
  bool active = t < nt;
  long probes = 0;
  bool placed = false;
  if (active) {
    const ScTriple me = sc_triple(tri, lead, t);
    active = me.ok;
    if (me.ok) {
      unsigned long s = (unsigned long)er_sc::triple_hash(me.k) & mask;
      for (unsigned long n = 0; n <= mask; n++, s = (s + 1) & mask) {
        probes++;
        int cur = sc_load(table + s);
        if (cur < 0) {
          cur = atomicCAS(table + s, -1, (int)t);
          if (cur < 0) {
            placed = true;
            break;
          }
        }
        const ScTriple o = sc_triple(tri, lead, cur);
        if (o.k[0] == me.k[0] && o.k[1] == me.k[1] && o.k[2] == me.k[2]) {
          if (cur > (int)t) atomicMin(table + s, (int)t);
          placed = true;
          break;
        }
      }
      if (placed) slot[t] = (unsigned)s;
    }
  }
  sc_report(probes, placed, active, diag, D_PROBE_T);
}

// Triangles, the two passes of er_compact.h.  A triangle is kept iff it is not degenerate and its slot holds its own index.  pass 0: used[L] = 1 for the leads a kept
// triangle names, blk[2 b ..] = kept and degenerate triangles of block b.  pass 1: behind the host's prefix (off[b]) the kept triangles in their
// order, with their own rotation: out = the ranks of their clusters, index_out = their input index.
__global__ __launch_bounds__(kScBlock) void k_st_compact(const int* __restrict__ tri, long nt, const int* __restrict__ lead, const int* __restrict__ table,
                                                         const unsigned* __restrict__ slot, int* __restrict__ used, long* __restrict__ blk,
                                                         const long* __restrict__ off, int pass, const int* __restrict__ rank, int* __restrict__ out,
                                                         int* __restrict__ index_out) {
  __shared__ int s_tally[2][kScBlock / 64];
  const long t = (long)blockIdx.x * kScBlock + threadIdx.x;
  int A = 0, B = 0, C = 0;
  bool keep = false, deg = false;
  if (t < nt) {
    A = lead[tri[3 * t]];
    B = lead[tri[3 * t + 1]];
    C = lead[tri[3 * t + 2]];
    deg = A == B || B == C || A == C;
    keep = !deg && table[slot[t]] == (int)t;
  }
  const BlockTally<kScBlock, 2> tally(s_tally, {keep, deg});
  if (!pass) {
    if (keep) used[A] = used[B] = used[C] = 1;
    tally.block_totals(blk);
    return;
  }
  if (!keep) return;
  const long o = tally.rank_in_block(off[blockIdx.x]);
  if (out) {
    out[3 * o] = rank[A];
    out[3 * o + 1] = rank[B];
    out[3 * o + 2] = rank[C];
  }
  if (index_out) index_out[o] = (int)t;
}

// Vertices, the same two passes.  A cluster is an output vertex iff a kept triangle names it; it is counted and written by its lead, so the output is in
// ascending order of lead.  pass 0: blk[2 b ..] = output vertices and leads (= occupied cells) of block b.  pass 1: rank[v] = the output index
// of the cluster v leads, or -1 (also for every v that leads nothing), and the finished rows where their arrays exist.
__global__ __launch_bounds__(kScBlock) void k_sv_compact(const int* __restrict__ lead, const int* __restrict__ used, long nv, long* __restrict__ blk,
                                                         const long* __restrict__ off, int pass, int* __restrict__ rank,
                                                         const unsigned long long* __restrict__ pos, const unsigned long long* __restrict__ nsum,
                                                         const unsigned long long* __restrict__ csum, float4* __restrict__ verts_out,
                                                         float4* __restrict__ nrm_out, uchar4* __restrict__ rgba_out, int* __restrict__ members_out) {
  __shared__ int s_tally[2][kScBlock / 64];
  const long v = (long)blockIdx.x * kScBlock + threadIdx.x;
  bool keep = false, leads = false;
  if (v < nv) {
    leads = lead[v] == (int)v;
    keep = leads && used[v] != 0;
  }
  const BlockTally<kScBlock, 2> tally(s_tally, {keep, leads});
  if (!pass) {
    tally.block_totals(blk);
    return;
  }
  if (v >= nv) return;
  const long o = tally.rank_in_block(off[blockIdx.x]);
  rank[v] = keep ? (int)o : -1;
  if (!keep) return;
  const long long n = (long long)pos[4 * v + 3];
  if (verts_out)
    verts_out[o] = make_float4(er_sc::finish_position((long long)pos[4 * v], n), er_sc::finish_position((long long)pos[4 * v + 1], n),
                               er_sc::finish_position((long long)pos[4 * v + 2], n), 0.0f);
  if (nrm_out) {
    float g[3];
    er_sc::finish_normal((long long)nsum[4 * v], (long long)nsum[4 * v + 1], (long long)nsum[4 * v + 2], (long long)nsum[4 * v + 3], g);
    nrm_out[o] = make_float4(g[0], g[1], g[2], 0.0f);
  }
  if (rgba_out) {
    const long long m = (long long)csum[4 * v + 3];
    uchar4 c = make_uchar4(0, 0, 0, 0);
    if (m > 0)
      c = make_uchar4((unsigned char)er_sc::finish_channel((long long)csum[4 * v], m), (unsigned char)er_sc::finish_channel((long long)csum[4 * v + 1], m),
                      (unsigned char)er_sc::finish_channel((long long)csum[4 * v + 2], m), 255);
    rgba_out[o] = c;
  }
  if (members_out) members_out[o] = (int)n;
}

__global__ __launch_bounds__(kScBlock) void k_sc_cluster(const int* __restrict__ lead, const int* __restrict__ rank, long nv, int* __restrict__ cluster) {
  const long v = (long)blockIdx.x * kScBlock + threadIdx.x;
  if (v < nv) cluster[v] = rank[lead[v]];
}

unsigned sc_grid(long n) { return (unsigned)((n + kScBlock - 1) / kScBlock); }

// slots of a table for n keys: a power of two, load at most 1/2
unsigned long sc_table_size(long n) {
  unsigned long size = 2;
  while (size < 2ul * (unsigned long)n) size <<= 1;
  return size;
}

}  // namespace

namespace er_tsdf_k {

// (declared in er_mesh.h)
int simplify_on_device(const char* who, hipStream_t s, const float4* d_verts, const float4* d_nrm, const uchar4* d_rgba, long nv, const int* d_tri, long nt,
                       float cell, const ScWant& want, const std::function<int(const ScMesh&)>& counted, er::DevScope& owned, ScMesh* out) {
  // the first offenders
  unsigned long long* d_first = nullptr;
  int* d_diag = nullptr;
  if (owned.alloc(&d_first, 2, who)) return 1;
  if (owned.alloc(&d_diag, D_COUNT, who)) return 1;
  ER_W(who, hipMemsetAsync(d_first, 0xFF, 2 * sizeof(unsigned long long), s));
  ER_W(who, hipMemsetAsync(d_diag, 0, D_COUNT * sizeof(int), s));
  hipLaunchKernelGGL(k_sc_check, dim3(sc_grid(std::max(nv, nt))), dim3(kScBlock), 0, s, d_verts, nv, cell, d_tri, nt, d_first);
  ER_W(who, hipGetLastError());
  unsigned long long first[2] = {kScNone, kScNone};
  ER_W(who, hipMemcpyAsync(first, d_first, sizeof first, hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  if (first[0] != kScNone) {
    const long v = (long)first[0];
    float p[4] = {0, 0, 0, 0};
    ER_W(who, hipMemcpy(p, d_verts + v, sizeof p, hipMemcpyDeviceToHost));
    if (er_sc::vertex_offence(p[0], p[1], p[2], cell) == 1)
      return er::fail("%s: vertex %ld (%g, %g, %g) has a coordinate that is not finite or not below 4096 m in magnitude", who, v, p[0], p[1], p[2]);
    return er::fail("%s: vertex %ld (%g, %g, %g) lies in cell (%.0f, %.0f, %.0f) of %g m, outside [-2^20, 2^20)", who, v, p[0], p[1], p[2],
                    er_sc::cell_of(p[0], cell), er_sc::cell_of(p[1], cell), er_sc::cell_of(p[2], cell), cell);
  }
  if (first[1] != kScNone) {
    const long t = (long)first[1];
    int k[3] = {0, 0, 0};
    ER_W(who, hipMemcpy(k, d_tri + 3 * t, sizeof k, hipMemcpyDeviceToHost));
    for (int q = 0; q < 3; q++)
      if (k[q] < 0 || (long)k[q] >= nv) return er::fail("%s: triangle %ld names vertex %d, outside [0, %ld)", who, t, k[q], nv);
  }

  // clusters, sums, duplicate triangles, the counting passes
  const unsigned long vsize = sc_table_size(nv), tsize = sc_table_size(nt);
  const long nbv = (long)sc_grid(nv), nbt = (long)sc_grid(nt);
  int *d_vtable = nullptr, *d_ttable = nullptr, *d_lead = nullptr, *d_used = nullptr, *d_rank = nullptr;
  unsigned *d_vslot = nullptr, *d_tslot = nullptr;
  unsigned long long *d_pos = nullptr, *d_nsum = nullptr, *d_csum = nullptr;
  TwoPass& lists = out->lists;
  const int lv = lists.add(nbv, 2), lt = lists.add(nbt, 2);
  if (owned.alloc(&d_vtable, vsize, who)) return 1;
  if (owned.alloc(&d_ttable, tsize, who)) return 1;
  if (owned.alloc(&d_vslot, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_tslot, (size_t)nt, who)) return 1;
  if (owned.alloc(&d_lead, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_used, (size_t)nv, who)) return 1;
  if (owned.alloc(&d_pos, (size_t)nv * 4, who)) return 1;
  if (lists.alloc(owned, who)) return 1;
  ER_W(who, hipMemsetAsync(d_vtable, 0xFF, vsize * sizeof(int), s));
  ER_W(who, hipMemsetAsync(d_ttable, 0xFF, tsize * sizeof(int), s));
  ER_W(who, hipMemsetAsync(d_vslot, 0, (size_t)nv * sizeof(unsigned), s));   // (a slot that an overflowing table leaves unset is still an address)
  ER_W(who, hipMemsetAsync(d_tslot, 0, (size_t)nt * sizeof(unsigned), s));
  ER_W(who, hipMemsetAsync(d_used, 0, (size_t)nv * sizeof(int), s));
  ER_W(who, hipMemsetAsync(d_pos, 0, (size_t)nv * 4 * sizeof(unsigned long long), s));
  const bool with_n = d_nrm && want.nrm, with_c = d_rgba && want.rgba;
  if (with_n) {
    if (owned.alloc(&d_nsum, (size_t)nv * 4, who)) return 1;
    ER_W(who, hipMemsetAsync(d_nsum, 0, (size_t)nv * 4 * sizeof(unsigned long long), s));
  }
  if (with_c) {
    if (owned.alloc(&d_csum, (size_t)nv * 4, who)) return 1;
    ER_W(who, hipMemsetAsync(d_csum, 0, (size_t)nv * 4 * sizeof(unsigned long long), s));
  }
  hipLaunchKernelGGL(k_sc_insert, dim3((unsigned)nbv), dim3(kScBlock), 0, s, d_verts, nv, cell, d_vtable, vsize - 1, d_vslot, d_diag);
  hipLaunchKernelGGL(k_sc_sums, dim3((unsigned)nbv), dim3(kScBlock), 0, s, d_verts, with_n ? d_nrm : nullptr, with_c ? d_rgba : nullptr, nv, d_vtable, d_vslot,
                     d_lead, d_pos, d_nsum, d_csum);
  hipLaunchKernelGGL(k_st_insert, dim3((unsigned)nbt), dim3(kScBlock), 0, s, d_tri, nt, d_lead, d_ttable, tsize - 1, d_tslot, d_diag);
  ER_W(who, hipGetLastError());
  float4 *d_verts_out = nullptr, *d_nrm_out = nullptr;
  uchar4* d_rgba_out = nullptr;
  int *d_members = nullptr, *d_tri_out = nullptr, *d_tri_index = nullptr;
  auto triangles = [&](int pass) {
    hipLaunchKernelGGL(k_st_compact, dim3((unsigned)nbt), dim3(kScBlock), 0, s, d_tri, nt, d_lead, d_ttable, d_tslot, d_used, lists.blk(lt), lists.off(lt), pass, d_rank,
                       d_tri_out, d_tri_index);
    ER_W(who, hipGetLastError());
    return 0;
  };
  auto vertices = [&](int pass) {
    hipLaunchKernelGGL(k_sv_compact, dim3((unsigned)nbv), dim3(kScBlock), 0, s, d_lead, d_used, nv, lists.blk(lv), lists.off(lv), pass, d_rank, d_pos, d_nsum, d_csum,
                       d_verts_out, d_nrm_out, d_rgba_out, d_members);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (triangles(0) || vertices(0)) return 1;
  int diag[D_COUNT] = {0, 0, 0, 0};
  if (lists.read_counts(who, s)) return 1;
  ER_W(who, hipMemcpyAsync(diag, d_diag, sizeof diag, hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  if (diag[D_FULL]) return er::fail("%s: a probe sequence ran through its whole table (%lu and %lu slots)", who, vsize, tsize);
  lists.prefix();
  const long nvk = lists.total(lv), ntk = lists.total(lt), cells = lists.total(lv, 1), degenerate = lists.total(lt, 1);
  out->nv = nvk;
  out->ntri = ntk;
  out->stats[0] = cells;
  out->stats[1] = degenerate;
  out->stats[2] = nt - degenerate - ntk;
  out->stats[3] = cells - nvk;
  out->probes[0] = diag[D_PROBE_V];
  out->probes[1] = diag[D_PROBE_T];
  if (counted(*out)) return 1;
  if (!want.any()) return 0;

  // the second passes
  if (lists.upload_offsets(who, s)) return 1;
  if (owned.alloc(&d_rank, (size_t)nv, who)) return 1;
  if (nvk > 0) {
    if (want.verts && owned.alloc(&d_verts_out, (size_t)nvk, who)) return 1;
    if (with_n && owned.alloc(&d_nrm_out, (size_t)nvk, who)) return 1;
    if (with_c && owned.alloc(&d_rgba_out, (size_t)nvk, who)) return 1;
    if (want.members && owned.alloc(&d_members, (size_t)nvk, who)) return 1;
  }
  if (vertices(1)) return 1;
  if (ntk > 0 && (want.tri || want.tri_index)) {
    if (want.tri && owned.alloc(&d_tri_out, (size_t)ntk * 3, who)) return 1;
    if (want.tri_index && owned.alloc(&d_tri_index, (size_t)ntk, who)) return 1;
    if (triangles(1)) return 1;
  }
  if (want.cluster) {
    if (owned.alloc(&out->d_cluster, (size_t)nv, who)) return 1;
    hipLaunchKernelGGL(k_sc_cluster, dim3((unsigned)nbv), dim3(kScBlock), 0, s, d_lead, d_rank, nv, out->d_cluster);
    ER_W(who, hipGetLastError());
  }
  out->d_verts = d_verts_out;
  out->d_nrm = d_nrm_out;
  out->d_rgba = d_rgba_out;
  out->d_members = d_members;
  out->d_tri = d_tri_out;
  out->d_tri_index = d_tri_index;
  return 0;
}

int sc_copy_back(const char* who, hipStream_t s, const ScMesh& r, long nv_in, float* verts, float* nrm, uint8_t* rgba, int* members, int* tri, int* tri_index,
                 int* cluster) {
  if (verts && r.d_verts) ER_W(who, hipMemcpyAsync(verts, r.d_verts, (size_t)r.nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (nrm && r.d_nrm) ER_W(who, hipMemcpyAsync(nrm, r.d_nrm, (size_t)r.nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (rgba && r.d_rgba) ER_W(who, hipMemcpyAsync(rgba, r.d_rgba, (size_t)r.nv * sizeof(uchar4), hipMemcpyDeviceToHost, s));
  if (members && r.d_members) ER_W(who, hipMemcpyAsync(members, r.d_members, (size_t)r.nv * sizeof(int), hipMemcpyDeviceToHost, s));
  if (tri && r.d_tri) ER_W(who, hipMemcpyAsync(tri, r.d_tri, (size_t)r.ntri * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  if (tri_index && r.d_tri_index) ER_W(who, hipMemcpyAsync(tri_index, r.d_tri_index, (size_t)r.ntri * sizeof(int), hipMemcpyDeviceToHost, s));
  if (cluster && r.d_cluster) ER_W(who, hipMemcpyAsync(cluster, r.d_cluster, (size_t)nv_in * sizeof(int), hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  return 0;
}

}  // namespace er_tsdf_k

extern "C" {

int er_mesh_simplify(const float* verts_host, const float* normals_host, const uint8_t* colors_host, long n_vertices, const int* tri_host,
                     long n_triangles, float cell, int device, float* verts_out, float* normals_out, uint8_t* colors_out, int* members_out,
                     long capacity_vertices, int* tri_out, int* tri_index_out, long capacity_triangles, int* cluster_out, long* n_vertices_out,
                     long* n_triangles_out, long stats[4], long probes[2]) {
  const char* who = "er_mesh_simplify";
  if (!n_vertices_out || !n_triangles_out || (n_vertices > 0 && !verts_host) || (n_triangles > 0 && !tri_host))
    return er::fail("er_mesh_simplify: NULL argument");
  if ((normals_out && !normals_host) || (colors_out && !colors_host))
    return er::fail("er_mesh_simplify: an output of normals or colours without the input to make it from");
  if (n_triangles < 0 || n_vertices < 0) return er::fail("er_mesh_simplify: %ld triangles, %ld vertices", n_triangles, n_vertices);
  if (n_vertices > (long)INT_MAX) return er::fail("er_mesh_simplify: %ld vertices; the limit is 2^31 - 1 (int32 indices)", n_vertices);
  if (n_triangles > (long)INT_MAX) return er::fail("er_mesh_simplify: %ld triangles; the limit is 2^31 - 1 (int32 slots)", n_triangles);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_mesh_simplify: no HIP device available (liber_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return er::fail("er_mesh_simplify: device %d of %d", device, ndev);
  if (!(std::isfinite(cell) && cell > 0.0f)) return er::fail("er_mesh_simplify: cell = %g m; it has to be finite and above 0", cell);
  const long nv = n_vertices, nt = n_triangles;
  if (nv == 0 || nt == 0) {                                    // the empty mesh: nothing to launch, no vertex is looked at
    *n_vertices_out = *n_triangles_out = 0;
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    if (probes) probes[0] = probes[1] = 0;
    if (cluster_out)
      for (long v = 0; v < nv; v++) cluster_out[v] = -1;
    return 0;
  }
  ER_HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;                                     // (the null stream: the call is synchronous)
  ScMesh r;                                                    // (before own: its lists outlive the copies that own's hipFree waits for)
  er::DevScope own;
  float4 *d_verts = nullptr, *d_nrm = nullptr;
  uchar4* d_rgba = nullptr;
  int* d_tri = nullptr;
  if (own.alloc(&d_verts, (size_t)nv, who)) return 1;
  if (own.alloc(&d_tri, (size_t)nt * 3, who)) return 1;
  ER_W(who, hipMemcpyAsync(d_verts, verts_host, (size_t)nv * sizeof(float4), hipMemcpyHostToDevice, s));
  ER_W(who, hipMemcpyAsync(d_tri, tri_host, (size_t)nt * 3 * sizeof(int), hipMemcpyHostToDevice, s));
  if (normals_out) {
    if (own.alloc(&d_nrm, (size_t)nv, who)) return 1;
    ER_W(who, hipMemcpyAsync(d_nrm, normals_host, (size_t)nv * sizeof(float4), hipMemcpyHostToDevice, s));
  }
  if (colors_out) {
    if (own.alloc(&d_rgba, (size_t)nv, who)) return 1;
    ER_W(who, hipMemcpyAsync(d_rgba, colors_host, (size_t)nv * sizeof(uchar4), hipMemcpyHostToDevice, s));
  }
  const ScWant want{verts_out != nullptr, normals_out != nullptr, colors_out != nullptr, members_out != nullptr, tri_out != nullptr, tri_index_out != nullptr,
                    cluster_out != nullptr};
  const bool want_rows = want.verts || want.nrm || want.rgba || want.members;
  auto counted = [&](const ScMesh& r) {
    *n_vertices_out = r.nv;
    *n_triangles_out = r.ntri;
    for (int q = 0; q < 4 && stats; q++) stats[q] = r.stats[q];
    for (int q = 0; q < 2 && probes; q++) probes[q] = r.probes[q];
    if (want_rows && capacity_vertices < r.nv) return er::fail("er_mesh_simplify: capacity %ld < %ld vertices", capacity_vertices, r.nv);
    if ((want.tri || want.tri_index) && capacity_triangles < r.ntri)
      return er::fail("er_mesh_simplify: capacity %ld < %ld triangles", capacity_triangles, r.ntri);
    return 0;
  };
  if (simplify_on_device(who, s, d_verts, d_nrm, d_rgba, nv, d_tri, nt, cell, want, counted, own, &r)) return 1;
  return sc_copy_back(who, s, r, nv, verts_out, normals_out, colors_out, members_out, tri_out, tri_index_out, cluster_out);
}

int er_tsdf_extract_mesh_simplified(er_tsdf_t h, float cell, long min_triangles, int largest_only, int want_colors, float* verts_host,
                                    float* normals_host, uint8_t* colors_host, int* members_host, long capacity_vertices, int* tri_host,
                                    long capacity_triangles, long* n_vertices, long* n_triangles, long stats[4], long before[2], long probes[2]) {
  const char* who = "er_tsdf_extract_mesh_simplified";
  if (!h || !n_vertices || !n_triangles) return er::fail("er_tsdf_extract_mesh_simplified: NULL argument");
  if (min_triangles < 0) return er::fail("er_tsdf_extract_mesh_simplified: min_triangles = %ld", min_triangles);
  if (colors_host && !want_colors) return er::fail("er_tsdf_extract_mesh_simplified: an output of colours without want_colors");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_tsdf_extract_mesh_simplified: no HIP device available (liber_hip has no CPU fallback)");
  if (!(std::isfinite(cell) && cell > 0.0f)) return er::fail("er_tsdf_extract_mesh_simplified: cell = %g m; it has to be finite and above 0", cell);
  ER_HIP_TRY(hipSetDevice(h->device));
  if (want_colors && color_sample_on_device(h, who, nullptr, 0, nullptr)) return 1;
  *n_vertices = *n_triangles = 0;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (before) before[0] = before[1] = 0;
  if (probes) probes[0] = probes[1] = 0;
  hipStream_t s = h->stream;

  // the unsimplified mesh, cleaned where that is asked for: it stays in device memory
  ScMesh r;                                                    // (r and c before m: their lists outlive the copies that m's hipFree waits for)
  CleanedMesh c;
  DeviceMesh m;
  const float4 *d_verts = nullptr, *d_nrm = nullptr;
  const int* d_tri = nullptr;
  long nv = 0, nt = 0;
  if (min_triangles > 1 || largest_only) {
    auto nothing = [](const CleanedMesh&) { return 0; };
    if (mesh_cleaned_on_device(h, who, min_triangles, largest_only, true, normals_host != nullptr, true, true, nothing, &m, &c)) return 1;
    nv = c.nv;
    nt = c.ntri;
    d_verts = c.d_verts;
    d_nrm = c.d_nrm;
    d_tri = c.d_tri;
  } else {
    auto limit = [&](long n, long) {
      if (n > (long)INT_MAX) return er::fail("er_tsdf_extract_mesh_simplified: %ld vertices; the limit is 2^31 - 1 (int32 indices)", n);
      return 0;
    };
    if (mesh_indexed_on_device(h, who, true, normals_host != nullptr, true, &nv, &nt, limit, &m)) return 1;
    d_verts = m.d_verts;
    d_nrm = m.d_nrm;
    d_tri = m.d_tri;
  }
  if (nv == 0 || nt == 0 || !d_verts || !d_tri) return 0;      // an empty volume, one without a crossing, or nothing left of it
  if (before) {
    before[0] = nv;
    before[1] = nt;
  }
  uchar4* d_rgba = nullptr;
  if (colors_host) {                                           // the colours of the unsimplified vertices, sampled where they lie
    if (m.owned.alloc(&d_rgba, (size_t)nv, who)) return 1;
    if (color_sample_on_device(h, who, d_verts, nv, d_rgba)) return 1;
  }
  const ScWant want{verts_host != nullptr, normals_host != nullptr, colors_host != nullptr, members_host != nullptr, tri_host != nullptr, false, false};
  const bool want_rows = want.verts || want.nrm || want.rgba || want.members;
  auto counted = [&](const ScMesh& r) {
    *n_vertices = r.nv;
    *n_triangles = r.ntri;
    for (int q = 0; q < 4 && stats; q++) stats[q] = r.stats[q];
    for (int q = 0; q < 2 && probes; q++) probes[q] = r.probes[q];
    if (want_rows && capacity_vertices < r.nv) return er::fail("er_tsdf_extract_mesh_simplified: capacity %ld < %ld vertices", capacity_vertices, r.nv);
    if (want.tri && capacity_triangles < r.ntri)
      return er::fail("er_tsdf_extract_mesh_simplified: capacity %ld < %ld triangles", capacity_triangles, r.ntri);
    return 0;
  };
  if (simplify_on_device(who, s, d_verts, d_nrm, d_rgba, nv, d_tri, nt, cell, want, counted, m.owned, &r)) return 1;
  return sc_copy_back(who, s, r, nv, verts_host, normals_host, colors_host, members_host, tri_host, nullptr, nullptr);
}

}  // extern "C"
