// er_mesh.h -- what the mesh translation units (er_mesh_cc.hip, er_mesh_simplify.hip, er_mesh_smooth.hip) and er_tsdf_color.hip know about each
// other: the device-to-device steps behind er_tsdf_extract_mesh_cleaned, er_mesh_simplify and er_tsdf_sample_colors, for
// er_tsdf_extract_mesh_simplified and er_tsdf_extract_mesh_smoothed to chain.  Internal: not part of the C ABI
// (include/er_hip.h).  Host code only: no kernel is declared here.
#pragma once

#include "er_tsdf.h"

namespace er_tsdf_k {

// The cleaned mesh of er_tsdf_extract_mesh_cleaned in device memory: every array belongs to the DeviceMesh it was made from (DeviceMesh::owned)
// and is NULL when it was not asked for or the cleaned mesh is empty.
struct CleanedMesh {
  long nv = 0, ntri = 0;                   // after filtering
  long stats[4] = {0, 0, 0, 0};            // components found, components kept, vertices dropped, triangles dropped
  float4 *d_verts = nullptr, *d_nrm = nullptr;
  int *d_index = nullptr, *d_tri = nullptr;
  TwoPass lists;                           // the vertex and the triangle list between their passes (er_compact.h)
};

// ---- er_mesh_cc.hip ----
// er_tsdf_extract_mesh_cleaned without the way back: extraction (mesh_indexed_on_device into *m; refusals of the unfiltered mesh under `who`),
// labelling, selection, the counting passes -- then c->nv, c->ntri and c->stats are set and counted(*c) is called, which refuses what the
// caller has to refuse (non-zero ends the call with 1) -- and the compaction of the rows asked for (want_rows: vertices, normals where they were
// extracted, index) and of the triangles (want_t).  An empty volume, an empty cleaned mesh, or nothing asked for returns 0 with the arrays NULL;
// counted is not called for an empty volume.  The kernels may still be in flight on h->stream on return.
__attribute__((visibility("hidden"))) int mesh_cleaned_on_device(er_tsdf_t h, const char* who, long min_triangles, int largest_only, bool want_v,
                                                                 bool want_n, bool want_rows, bool want_t,
                                                                 const std::function<int(const CleanedMesh&)>& counted, DeviceMesh* m, CleanedMesh* c);

// ---- er_mesh_simplify.hip, for er_mesh_smooth.hip ----
struct ScWant {
  bool verts, nrm, rgba, members, tri, tri_index, cluster;
  bool any() const { return verts || nrm || rgba || members || tri || tri_index || cluster; }
};

// What the clustering leaves in device memory: every array belongs to `owned` of the call and is NULL when it was not asked for.
struct ScMesh {
  long nv = 0, ntri = 0;
  long stats[4] = {0, 0, 0, 0};
  long probes[2] = {0, 0};
  float4 *d_verts = nullptr, *d_nrm = nullptr;
  uchar4* d_rgba = nullptr;
  int *d_members = nullptr, *d_tri = nullptr, *d_tri_index = nullptr, *d_cluster = nullptr;
  TwoPass lists;                                               // the vertex and the triangle list between their passes
};

// The clustering of nv > 0 vertices (d_nrm, d_rgba nullable) and nt > 0 triangles in device memory, on stream s, which it synchronises twice.
// The refusals of the input come first; then the counts and stats are set and counted(*out) refuses what the caller has to refuse (non-zero
// ends the call with 1); then the arrays of `want` are made.  Temporaries and results go to `owned`.
__attribute__((visibility("hidden"))) int simplify_on_device(const char* who, hipStream_t s, const float4* d_verts, const float4* d_nrm, const uchar4* d_rgba,
                                                             long nv, const int* d_tri, long nt, float cell, const ScWant& want,
                                                             const std::function<int(const ScMesh&)>& counted, er::DevScope& owned, ScMesh* out);

// The way back of whatever simplify_on_device left, on stream s, which it synchronises.
__attribute__((visibility("hidden"))) int sc_copy_back(const char* who, hipStream_t s, const ScMesh& r, long nv_in, float* verts, float* nrm, uint8_t* rgba,
                                                       int* members, int* tri, int* tri_index, int* cluster);

// ---- er_tsdf_color.hip ----
// er_tsdf_sample_colors between two device arrays, enqueued on h->stream: n float4 points -> n rgba.  Refuses, under `who`, what
// er_tsdf_sample_colors refuses of the volume (colour not enabled, a sharded volume, an overflowed pool); n == 0 is that check alone.
__attribute__((visibility("hidden"))) int color_sample_on_device(er_tsdf_t h, const char* who, const float4* d_points, long n, uchar4* d_rgba);

}  // namespace er_tsdf_k
