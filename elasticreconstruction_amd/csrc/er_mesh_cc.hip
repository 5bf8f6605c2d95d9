// er_mesh_cc.hip -- connected components of an indexed triangle mesh and the mesh cleaned of its small ones (the definitions
// stand in include/er_hip.h above er_mesh_components).  A translation unit of its own: nothing here is compiled into the code object of
// er_tsdf_extract.hip, whose kernels produce the mesh this file works on (er_tsdf.h: mesh_indexed_on_device).
//
// Labelling is a loop of launches.  A round is k_cc_hook -- per triangle the minimum m of its three labels goes, by atomicMin, into every
// label that differs from m and into that label's own label (its parent) -- and, if the hook moved anything, k_cc_jump, which sends every
// label to the end of its chain.  Invariants: label[v] <= v, and label[v] is a vertex of v's component (a label is only ever replaced by a
// label read from the same triangle or the same chain).  A hook launch that moves nothing has read, for every triangle, three equal labels
// while nobody wrote: all labels of a component are then one value L, L belongs to the component, so label[L] = L, and the component's
// smallest vertex u has label[u] <= u inside the component, so L = u.  That quiet launch is the proof of the fixed point; the host reads one
// word per round to learn of it.  Inside a launch other workgroups' labels are touched only by agent-scope atomics and relaxed agent-scope
// atomic loads, every value only ever decreases, and a value read late costs at most a round: no fence, no flag, no grid synchronisation
// hands anything over inside a launch -- the launch boundary publishes the rest.
#include "er_mesh.h"

#include <climits>

namespace {

using namespace er_tsdf_k;

constexpr int kCcBlock = 256;
// The round loop's cap: a bug ends as a refusal that names the count, not as a hang.  The fixtures of tests/test_mesh_components_gpu.py
// need at most 15 rounds on the device (the bit-reversed strip of 65 537 triangles; profiles/mesh_clean.txt).
constexpr int kCcMaxRounds = 1024;

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(kCcBlock) void k_cc_init(int* __restrict__ label, long nv) {
  const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
  if (v < nv) label[v] = (int)v;
}

// One thread per triangle.  changed: the word the host reads; a wave that moved a label stores the round's number in it.
__global__ __launch_bounds__(kCcBlock) void k_cc_hook(const int* __restrict__ tri, long nt, int* label, int* changed, int round) {
  const long t = (long)blockIdx.x * kCcBlock + threadIdx.x;
  bool moved = false;
  if (t < nt) {
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const int la = cc_load(label + a), lb = cc_load(label + b), lc = cc_load(label + c);
    const int m = min(la, min(lb, lc));
    if (la != m) {
      atomicMin(label + la, m);
      atomicMin(label + a, m);
      moved = true;
    }
    if (lb != m) {
      atomicMin(label + lb, m);
      atomicMin(label + b, m);
      moved = true;
    }
    if (lc != m) {
      atomicMin(label + lc, m);
      atomicMin(label + c, m);
      moved = true;
    }
  }
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) __hip_atomic_store(changed, round, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One thread per vertex: label[v] follows its chain to the end.  The chain strictly descends (label[x] <= x), so the walk ends; every step is
// published at once, so that the walks of higher vertices, which lead through lower ones, find short chains.
__global__ __launch_bounds__(kCcBlock) void k_cc_jump(int* label, long nv) {
  const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
  if (v >= nv) return;
  int l = cc_load(label + v);
  for (;;) {
    const int p = cc_load(label + l);
    if (p == l) break;
    atomicMin(label + v, p);
    l = p;
  }
}

// Triangles per root: a wave sends ONE add per distinct root among its 64 triangles (the mesh of a room is essentially one component: an add
// per triangle would queue them all on one word).
__global__ __launch_bounds__(kCcBlock) void k_cc_count(const int* __restrict__ tri, long nt, const int* __restrict__ label,
                                                       unsigned long long* __restrict__ cnt) {
  const long t = (long)blockIdx.x * kCcBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int r = t < nt ? label[tri[3 * t]] : -1;
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int rl = __shfl(r, lead);
    const unsigned long long same = __ballot(r == rl);
    if (lane == lead) atomicAdd(cnt + rl, (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(kCcBlock) void k_cc_vertex_count(const int* __restrict__ label, const unsigned long long* __restrict__ cnt, long nv,
                                                              long* __restrict__ out) {
  const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
  if (v < nv) out[v] = (long)cnt[label[v]];
}

// The largest component: the maximum over the roots of count << 31 | (2^31 - 1 - label), so that a tie goes to the smaller label.  A root's
// key is never 0 (label <= 2^31 - 2); *best starts as 0.
__global__ __launch_bounds__(kCcBlock) void k_cc_largest(const int* __restrict__ label, const unsigned long long* __restrict__ cnt, long nv,
                                                         unsigned long long* best) {
  const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
  unsigned long long key = 0ull;
  if (v < nv && label[v] == (int)v) key = cnt[v] << 31 | (unsigned long long)(0x7FFFFFFF - (int)v);
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

__device__ __forceinline__ bool cc_keep(const unsigned long long* __restrict__ cnt, int l, long min_tri, int best) {
  return (long)cnt[l] >= min_tri && (best < 0 || l == best);
}

// Vertices, the two passes of er_compact.h with three tallies.  pass 0: blk[3 b ..] = kept vertices, roots, kept roots of block b.  pass 1: behind
// the host's prefix over the first of these (off[b]) the kept vertices move, in their order: remap[v] = the new index or -1, index_out[new] = v,
// and the float4 rows of verts / nrm where those arrays exist.
__global__ __launch_bounds__(kCcBlock) void k_cc_vertices(const int* __restrict__ label, const unsigned long long* __restrict__ cnt, long nv, long min_tri,
                                                          int best, long* __restrict__ blk, const long* __restrict__ off, int pass,
                                                          int* __restrict__ remap, int* __restrict__ index_out, const float4* __restrict__ verts,
                                                          float4* __restrict__ verts_out, const float4* __restrict__ nrm, float4* __restrict__ nrm_out) {
  __shared__ int s_tally[3][kCcBlock / 64];
  const long v = (long)blockIdx.x * kCcBlock + threadIdx.x;
  bool keep = false, root = false;
  if (v < nv) {
    const int l = label[v];
    keep = cc_keep(cnt, l, min_tri, best);
    root = l == (int)v;
  }
  const BlockTally<kCcBlock, 3> tally(s_tally, {keep, root, keep && root});
  if (!pass) {
    tally.block_totals(blk);
    return;
  }
  if (v >= nv) return;
  const long o = tally.rank_in_block(off[blockIdx.x]);
  remap[v] = keep ? (int)o : -1;
  if (keep) {
    index_out[o] = (int)v;
    if (verts_out) verts_out[o] = verts[v];
    if (nrm_out) nrm_out[o] = nrm[v];
  }
}

// Triangles: a triangle is kept iff its vertices are, and they share one component.  pass 0: blk[b] = kept triangles of block b; pass 1: the
// kept triangles in their order with remapped indices.
__global__ __launch_bounds__(kCcBlock) void k_cc_triangles(const int* __restrict__ tri, long nt, const int* __restrict__ label,
                                                           const unsigned long long* __restrict__ cnt, long min_tri, int best, long* __restrict__ blk,
                                                           const long* __restrict__ off, int pass, const int* __restrict__ remap, int* __restrict__ out) {
  __shared__ int s_tally[1][kCcBlock / 64];
  const long t = (long)blockIdx.x * kCcBlock + threadIdx.x;
  int a = 0, b = 0, c = 0;
  bool keep = false;
  if (t < nt) {
    a = tri[3 * t];
    b = tri[3 * t + 1];
    c = tri[3 * t + 2];
    keep = cc_keep(cnt, label[a], min_tri, best);
  }
  const BlockTally<kCcBlock, 1> tally(s_tally, {keep});
  if (!pass) {
    tally.block_totals(blk);
    return;
  }
  if (!keep) return;
  const long o = tally.rank_in_block(off[blockIdx.x]);
  out[3 * o] = remap[a];
  out[3 * o + 1] = remap[b];
  out[3 * o + 2] = remap[c];
}

unsigned cc_grid(long n) { return (unsigned)((n + kCcBlock - 1) / kCcBlock); }

// Labels and triangles per root of the nt > 0 triangles d_tri over nv > 0 vertices, on stream s: d_label[nv], d_cnt[nv] (the count at the
// root's index, 0 elsewhere), d_word a device int.  Synchronises s.  *rounds = hook launches, the quiet one included.
int cc_label(const char* who, hipStream_t s, const int* d_tri, long nt, long nv, int* d_label, unsigned long long* d_cnt, int* d_word, int* rounds) {
  ER_W(who, hipMemsetAsync(d_word, 0, sizeof(int), s));
  ER_W(who, hipMemsetAsync(d_cnt, 0, (size_t)nv * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(nv)), dim3(kCcBlock), 0, s, d_label, nv);
  ER_W(who, hipGetLastError());
  int r = 0;
  for (;;) {
    if (r == kCcMaxRounds) return er::fail("%s: the labelling did not settle in %d rounds", who, r);
    r++;
    int word = 0;
    hipLaunchKernelGGL(k_cc_hook, dim3(cc_grid(nt)), dim3(kCcBlock), 0, s, d_tri, nt, d_label, d_word, r);
    ER_W(who, hipGetLastError());
    ER_W(who, hipMemcpyAsync(&word, d_word, sizeof(int), hipMemcpyDeviceToHost, s));
    ER_W(who, hipStreamSynchronize(s));
    if (word != r) break;
    hipLaunchKernelGGL(k_cc_jump, dim3(cc_grid(nv)), dim3(kCcBlock), 0, s, d_label, nv);
    ER_W(who, hipGetLastError());
  }
  *rounds = r;
  hipLaunchKernelGGL(k_cc_count, dim3(cc_grid(nt)), dim3(kCcBlock), 0, s, d_tri, nt, d_label, d_cnt);
  ER_W(who, hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int er_mesh_components(const int* tri_host, long n_triangles, long n_vertices, int device, int* label_host, long* count_host, long* n_components,
                       int* rounds) {
  const char* who = "er_mesh_components";
  if (!n_components || (n_triangles > 0 && !tri_host)) return er::fail("er_mesh_components: NULL argument");
  if (n_triangles < 0 || n_vertices < 0) return er::fail("er_mesh_components: %ld triangles, %ld vertices", n_triangles, n_vertices);
  if (n_vertices > (long)INT_MAX) return er::fail("er_mesh_components: %ld vertices; the limit is 2^31 - 1 (int32 indices)", n_vertices);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_mesh_components: no HIP device available (liber_hip has no CPU fallback)");
  if (device < 0 || device >= ndev) return er::fail("er_mesh_components: device %d of %d", device, ndev);
  // before any kernel uses an index as an address: the first triangle, in triangle order, that names no vertex
  for (long t = 0; t < n_triangles; t++)
    for (int q = 0; q < 3; q++) {
      const int i = tri_host[3 * t + q];
      if (i < 0 || (long)i >= n_vertices)
        return er::fail("er_mesh_components: triangle %ld names vertex %d, outside [0, %ld)", t, i, n_vertices);
    }
  const long nt = n_triangles, nv = n_vertices;
  if (nt == 0) {                                             // every vertex is a component of its own: nothing to launch
    for (long v = 0; v < nv; v++) {
      if (label_host) label_host[v] = (int)v;
      if (count_host) count_host[v] = 0;
    }
    *n_components = nv;
    if (rounds) *rounds = 0;
    return 0;
  }
  ER_HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;                                   // (the null stream: the call is synchronous)
  TwoPass lists;                                             // (only the count pass: the roots are its second tally; outlives `own`)
  er::DevScope own;
  int *d_tri = nullptr, *d_label = nullptr, *d_word = nullptr;
  unsigned long long* d_cnt = nullptr;
  long* d_vcnt = nullptr;
  const long nblk = (long)cc_grid(nv);
  const int lv = lists.add(nblk, 3);
  if (own.alloc(&d_tri, (size_t)nt * 3, who)) return 1;
  if (own.alloc(&d_label, (size_t)nv, who)) return 1;
  if (own.alloc(&d_cnt, (size_t)nv, who)) return 1;
  if (own.alloc(&d_word, 1, who)) return 1;
  if (lists.alloc(own, who)) return 1;
  ER_W(who, hipMemcpyAsync(d_tri, tri_host, (size_t)nt * 3 * sizeof(int), hipMemcpyHostToDevice, s));
  int r = 0;
  if (cc_label(who, s, d_tri, nt, nv, d_label, d_cnt, d_word, &r)) return 1;
  hipLaunchKernelGGL(k_cc_vertices, dim3((unsigned)nblk), dim3(kCcBlock), 0, s, d_label, d_cnt, nv, 0L, -1, lists.blk(lv), lists.off(lv), 0,
                     (int*)nullptr, (int*)nullptr, (const float4*)nullptr, (float4*)nullptr, (const float4*)nullptr, (float4*)nullptr);
  ER_W(who, hipGetLastError());
  if (lists.read_counts(who, s)) return 1;
  if (count_host) {
    if (own.alloc(&d_vcnt, (size_t)nv, who)) return 1;
    hipLaunchKernelGGL(k_cc_vertex_count, dim3((unsigned)nblk), dim3(kCcBlock), 0, s, d_label, d_cnt, nv, d_vcnt);
    ER_W(who, hipGetLastError());
    ER_W(who, hipMemcpyAsync(count_host, d_vcnt, (size_t)nv * sizeof(long), hipMemcpyDeviceToHost, s));
  }
  if (label_host) ER_W(who, hipMemcpyAsync(label_host, d_label, (size_t)nv * sizeof(int), hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  lists.prefix();
  *n_components = lists.total(lv, 1);
  if (rounds) *rounds = r;
  return 0;
}

int er_tsdf_extract_mesh_cleaned(er_tsdf_t h, long min_triangles, int largest_only, float* verts_host, float* normals_host, int* index_host,
                                 long capacity_vertices, int* tri_host, long capacity_triangles, long* n_vertices, long* n_triangles, long stats[4]) {
  const char* who = "er_tsdf_extract_mesh_cleaned";
  if (!h || !n_vertices || !n_triangles) return er::fail("er_tsdf_extract_mesh_cleaned: NULL argument");
  if (min_triangles < 0) return er::fail("er_tsdf_extract_mesh_cleaned: min_triangles = %ld", min_triangles);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return er::fail("er_tsdf_extract_mesh_cleaned: no HIP device available (liber_hip has no CPU fallback)");
  ER_HIP_TRY(hipSetDevice(h->device));
  *n_vertices = *n_triangles = 0;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  const bool want_v = verts_host || normals_host, want_rows = want_v || index_host;
  hipStream_t s = h->stream;
  CleanedMesh c;                                             // (before m: its lists outlive the copies that m's hipFree waits for)
  DeviceMesh m;
  auto counted = [&](const CleanedMesh& k) {
    *n_vertices = k.nv;
    *n_triangles = k.ntri;
    if (stats)
      for (int q = 0; q < 4; q++) stats[q] = k.stats[q];
    if (want_rows && capacity_vertices < k.nv) return er::fail("er_tsdf_extract_mesh_cleaned: capacity %ld < %ld vertices", capacity_vertices, k.nv);
    if (tri_host && capacity_triangles < k.ntri) return er::fail("er_tsdf_extract_mesh_cleaned: capacity %ld < %ld triangles", capacity_triangles, k.ntri);
    return 0;
  };
  if (mesh_cleaned_on_device(h, who, min_triangles, largest_only, want_v, normals_host != nullptr, want_rows, tri_host != nullptr, counted, &m, &c)) return 1;
  if (!c.d_index) return 0;                                  // (nothing has been written to the host)
  if (verts_host) ER_W(who, hipMemcpyAsync(verts_host, c.d_verts, (size_t)c.nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (normals_host) ER_W(who, hipMemcpyAsync(normals_host, c.d_nrm, (size_t)c.nv * sizeof(float4), hipMemcpyDeviceToHost, s));
  if (index_host) ER_W(who, hipMemcpyAsync(index_host, c.d_index, (size_t)c.nv * sizeof(int), hipMemcpyDeviceToHost, s));
  if (c.d_tri) ER_W(who, hipMemcpyAsync(tri_host, c.d_tri, (size_t)c.ntri * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  ER_W(who, hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"

namespace er_tsdf_k {

int mesh_cleaned_on_device(er_tsdf_t h, const char* who, long min_triangles, int largest_only, bool want_v, bool want_n, bool want_rows, bool want_t,
                           const std::function<int(const CleanedMesh&)>& counted, DeviceMesh* mesh, CleanedMesh* c) {
  DeviceMesh& m = *mesh;
  hipStream_t s = h->stream;
  auto limit = [&](long nv, long) {
    if (nv > (long)INT_MAX) return er::fail("%s: %ld vertices; the limit is 2^31 - 1 (int32 indices)", who, nv);
    return 0;
  };
  long nv = 0, nt = 0;                                       // (of the unfiltered mesh; the caller's counts are those after filtering)
  if (mesh_indexed_on_device(h, who, want_v, want_n, true, &nv, &nt, limit, &m)) return 1;
  if (nv == 0 || nt == 0 || !m.d_tri) return 0;              // an empty volume, or one without a crossing

  // labels, triangles per root, the largest component
  int *d_label = nullptr, *d_word = nullptr;
  unsigned long long *d_cnt = nullptr, *d_best = nullptr;
  if (m.owned.alloc(&d_label, (size_t)nv, who)) return 1;
  if (m.owned.alloc(&d_cnt, (size_t)nv, who)) return 1;
  if (m.owned.alloc(&d_word, 1, who)) return 1;
  int r = 0, best = -1;
  if (cc_label(who, s, m.d_tri, nt, nv, d_label, d_cnt, d_word, &r)) return 1;
  if (largest_only) {
    unsigned long long key = 0ull;
    if (m.owned.alloc(&d_best, 1, who)) return 1;
    ER_W(who, hipMemsetAsync(d_best, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_cc_largest, dim3(cc_grid(nv)), dim3(kCcBlock), 0, s, d_label, d_cnt, nv, d_best);
    ER_W(who, hipGetLastError());
    ER_W(who, hipMemcpyAsync(&key, d_best, sizeof(key), hipMemcpyDeviceToHost, s));
    ER_W(who, hipStreamSynchronize(s));
    best = 0x7FFFFFFF - (int)(key & 0x7FFFFFFFull);
  }

  // what stays: counts per block, offsets on the host
  const long nbv = (long)cc_grid(nv), nbt = (long)cc_grid(nt);
  TwoPass& lists = c->lists;
  const int lv = lists.add(nbv, 3), lt = lists.add(nbt, 1);
  if (lists.alloc(m.owned, who)) return 1;
  int *d_remap = nullptr, *d_index = nullptr, *d_tri_out = nullptr;
  float4 *d_verts_out = nullptr, *d_nrm_out = nullptr;
  auto vertices = [&](int pass) {
    hipLaunchKernelGGL(k_cc_vertices, dim3((unsigned)nbv), dim3(kCcBlock), 0, s, d_label, d_cnt, nv, min_triangles, best, lists.blk(lv), lists.off(lv), pass,
                       d_remap, d_index, m.d_verts, d_verts_out, m.d_nrm, d_nrm_out);
    ER_W(who, hipGetLastError());
    return 0;
  };
  auto triangles = [&](int pass) {
    hipLaunchKernelGGL(k_cc_triangles, dim3((unsigned)nbt), dim3(kCcBlock), 0, s, m.d_tri, nt, d_label, d_cnt, min_triangles, best, lists.blk(lt), lists.off(lt), pass,
                       d_remap, d_tri_out);
    ER_W(who, hipGetLastError());
    return 0;
  };
  if (vertices(0) || triangles(0)) return 1;
  if (lists.read_counts(who, s)) return 1;
  ER_W(who, hipStreamSynchronize(s));
  lists.prefix();
  const long nvk = lists.total(lv), ntk = lists.total(lt);
  c->nv = nvk;
  c->ntri = ntk;
  c->stats[0] = lists.total(lv, 1);                          // roots
  c->stats[1] = lists.total(lv, 2);                          // kept roots
  c->stats[2] = nv - nvk;
  c->stats[3] = nt - ntk;
  if (counted(*c)) return 1;
  if (nvk == 0 || (!want_rows && !want_t)) return 0;

  // the second passes
  if (lists.upload_offsets(who, s)) return 1;
  if (m.owned.alloc(&d_remap, (size_t)nv, who)) return 1;
  if (m.owned.alloc(&d_index, (size_t)nvk, who)) return 1;
  if (m.d_verts && m.owned.alloc(&d_verts_out, (size_t)nvk, who)) return 1;
  if (m.d_nrm && m.owned.alloc(&d_nrm_out, (size_t)nvk, who)) return 1;
  if (vertices(1)) return 1;
  if (want_t && ntk > 0) {
    if (m.owned.alloc(&d_tri_out, (size_t)ntk * 3, who)) return 1;
    if (triangles(1)) return 1;
  }
  c->d_verts = d_verts_out;
  c->d_nrm = d_nrm_out;
  c->d_index = d_index;
  c->d_tri = d_tri_out;
  return 0;
}

}  // namespace er_tsdf_k
