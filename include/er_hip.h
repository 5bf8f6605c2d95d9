/* er_hip.h -- C ABI of liber_hip.so, the MI355X (gfx950) implementation of the two data-parallel
 * stages of qianyizh/ElasticReconstruction:
 *
 *   path A  TSDF depth integration with control-grid warp   (reference: Integrate/)
 *   path B  pairwise ICP refinement + correspondences       (reference: BuildCorrespondence/)
 * and, after those two, the first rows of SURVEY.md 8f:
 *   RansacCurvature::getFitness / getInformation             (reference: GlobalRegistration/RansacCurvature.h)
 *   COptApp's per-point state, Hessian assembly and solve    (reference: FragmentOptimizer/OptApp.cpp, PointCloud.h)
 *
 * The reference has no FFI; its boundary is "executable + argv + files" (SURVEY.md 8b).  These
 * entry points are the thin C ABI the new host programs (and any cgo/JNI/ctypes caller) bind.
 * Each one cites the reference method it replaces.  Conventions:
 *   - plain C types only; 4x4 matrices are ROW-MAJOR arrays of 16 (double unless stated);
 *   - every function returns 0 on success, non-zero on failure; er_last_error() (thread-local)
 *     explains the last failure; nothing throws across the ABI;
 *   - handles are opaque and owned by the caller; calls on ONE handle must be serialised by the
 *     caller, different handles may be driven from different host threads (this mirrors the
 *     reference's "one OpenMP thread per pair" model, CorresApp.cpp:121,220);
 *   - "host" pointers are ordinary host memory, "dev" pointers are HIP device memory on the
 *     handle's device; there is NO CPU fallback: without a usable HIP device every constructor
 *     fails with an error.
 */
#ifndef ER_HIP_H_
#define ER_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ER_UNIT_RES 64                 /* TSDFVolume.cpp:57: new TSDFVolumeUnit( 64, ... ) */
#define ER_UNIT_VOX (64 * 64 * 64)
#define ER_MAX_BATCH 64                /* frames fused per launch (one bit each in a 64-bit mask) */

/* ------------------------------------------------------------------ misc ---- */
const char* er_last_error(void);
int er_device_count(void);                       /* number of visible HIP devices (0 if none) */
int er_abi_version(void);
/* OPT-IN, call before the process's first HIP call: asks the HIP runtime for n hardware queues (GPU_MAX_HW_QUEUES, default 4;
 * n <= 0 means 8) without overriding a value the user exported; returns the value in force.  A TSDF volume overlaps four
 * streams and runs ~15 % slower when two of them share a queue.  The library never sets this on its own (it would change the
 * queue set-up of every GPU user of the process): the drop-in programs and bench.py call it first thing in main(). */
int er_request_hw_queues(int n);

/* Page-locked host memory.  Every "host" pointer of this ABI may be ordinary (pageable) memory; result buffers
 * that come from er_host_alloc are written by asynchronous device-to-host copies without a staging pass. */
void* er_host_alloc(size_t bytes);               /* NULL on failure (see er_last_error) */
int er_host_free(void* p);
int er_host_copy_h2d(void* dev_dst, const void* host_src, size_t bytes);   /* blocking host -> device copy (current device) */
/* Device memory for hosts that do not speak HIP themselves: the list buffers of er_find_correspondence_batch / er_registration_batch
 * may live in HBM (the lists then never cross PCIe) and er_fopt_set_correspondences_dev consumes them there; er_device_copy_d2h fetches
 * one when a corres_<i>_<j>.txt is to be written after all. */
void* er_device_alloc(size_t bytes, int device);  /* NULL on failure */
int er_device_free(void* p);
int er_device_copy_d2h(void* host_dst, const void* dev_src, size_t bytes);   /* blocking device -> host copy */

/* ------------------------------------------------------------ path A: TSDF ---- */
typedef struct er_tsdf_s* er_tsdf_t;

/* Control-grid warp inputs for a batch of n frames (CIntegrateApp::Reproject, IntegrateApp.cpp:228-269).
 * All pointers are HOST memory. */
typedef struct er_warp {
  const float* ctr;         /* num_grids * (resolution+1)^3 * 3 floats; vertex i + j*(res+1) + k*(res+1)^2
                               (ControlGrid.h:41-43; file order of ControlGrid::Load, ControlGrid.cpp:15-34) */
  int num_grids;            /* --num        (IntegrateApp.h:70 ctr_num_) */
  int resolution;           /* --resolution (IntegrateApp.h:68) */
  float length;             /* --length, stored as float by ControlGrid::Load (ControlGrid.cpp:17-18) */
  const int* grid_index;    /* n ints: chunk = (frame_id-1)/interval of each frame (IntegrateApp.cpp:242) */
  const double* seg;        /* n * 16: seg_traj_[frame_id-1] (IntegrateApp.cpp:251) */
  const double* madj;       /* n * 16: traj[f-1]^-1 * traj[0] * seg[0]^-1 (IntegrateApp.cpp:243) */
} er_warp;

/* TSDFVolume::TSDFVolume( cols, rows ) + CameraParam (TSDFVolume.cpp:7-13, TSDFVolumeUnit.h:65-70).
 * cam6 = fx fy cx cy ICP_trunc integration_trunc (NULL = reference defaults 525 525 319.5 239.5 2.5 2.5).
 * max_units = capacity of the 64^3 volume-unit pool in HBM (2 MiB each, zero-filled up front). */
int er_tsdf_create(int cols, int rows, const float cam6[6], int max_units, int device, er_tsdf_t* out);
int er_tsdf_destroy(er_tsdf_t h);

/* Order the handle's work with an existing hipStream_t (e.g. torch's current stream): every call but the batch pipeline runs on it.
 * NULL = the handle's own stream.  (The pre-passes always use two internal auxiliary streams and the voxel pass the handle's own stream,
 * so that the three never share a hardware queue; the voxel passes of er_tsdf_integrate_frames wait for what the stream held when the
 * call began, and the stream waits for them before the handle uses it for the volume again.) */
int er_tsdf_set_stream(er_tsdf_t h, void* hip_stream);
int er_tsdf_synchronize(er_tsdf_t h);

/* TSDFVolume::ScaleDepth (TSDFVolume.cpp:19-36): depth uint16[rows*cols] -> scaled float[rows*cols]. */
int er_tsdf_scale_depth(er_tsdf_t h, const uint16_t* depth_host, float* scaled_host);

/* CIntegrateApp::Reproject pixel loop (IntegrateApp.cpp:236-268) for ONE frame, in place on host memory. */
int er_tsdf_reproject(er_tsdf_t h, uint16_t* depth_inout_host, const float* ctr_host, int resolution, float length,
                      const double seg[16], const double madj[16]);

/* One frame of CIntegrateApp::Execute's numeric tail (IntegrateApp.cpp:224-225):
 * ScaleDepth + TSDFVolume::Integrate (TSDFVolume.cpp:38-67 -> IntegrateVolumeUnit :69-102). */
int er_tsdf_integrate(er_tsdf_t h, const uint16_t* depth_host, const double T[16]);

/* n frames in order: [Reproject] + ScaleDepth + Integrate for each (IntegrateApp.cpp:217-225).
 * Results are identical to n sequential er_tsdf_integrate calls; internally frames are fused
 * ER_MAX_BATCH at a time so each voxel is read and written once per batch.
 * depth: n*rows*cols uint16, host memory if depth_on_device == 0 else device memory (left untouched).
 * Device depth must be COMPLETE when the call is made (synchronise the stream that produced it): the
 * per-pixel pre-passes of the next two batches run on the handle's two auxiliary streams so that they overlap each other
 * and the voxel pass of the previous batch, and those streams do not wait for the caller's (er_tsdf_wait_event).
 * T: n*16 host doubles (traj_[frame_id-1]).  warp may be NULL (rigid, --ref_traj). */
int er_tsdf_integrate_frames(er_tsdf_t h, int n, const uint16_t* depth, int depth_on_device, const double* T,
                             const er_warp* warp);

/* Test hook: ONE batch (1 <= n <= ER_MAX_BATCH frames; arguments as er_tsdf_integrate_frames) through the ordinary pipeline on a quiet handle
 * -- it is integrated into the volume like any other -- and then what the batch's voxel pass was given by the pre-pass, copied to the host:
 *   scaled        float[n * (rows*cols + *scaled_pad)]: the scaled depth of each frame followed by the frame's pad;
 *   tile_max/lo   float[tiles32 * ER_MAX_BATCH] each, [tile][frame], tiles32 = ceil(cols/32) * ceil(rows/32), row-major (columns of frames >= n
 *                 hold whatever earlier batches left);
 *   tile_lo_fine  float[tiles16 * ER_MAX_BATCH], [tile][frame], tiles16 = ceil(cols/16) * ceil(rows/16);
 *   keys, masks   the batch's units in ascending key order and the frames that touch each (bit f = frame f); at most keys_cap are
 *                 written, *n_keys is the number the batch has.
 * Any output pointer may be NULL.  The kernels are the ones every batch runs: the hook adds no argument and no branch to them. */
int er_tsdf_prepass_trace(er_tsdf_t h, int n, const uint16_t* depth, int depth_on_device, const double* T, const er_warp* warp,
                          float* scaled, int* scaled_pad, float* tile_max, float* tile_lo, float* tile_lo_fine,
                          int* keys, unsigned long long* masks, int keys_cap, int* n_keys);

/* Test hook: sets the use counter of one of the handle's reprojection z-buffers on a quiet handle -- which = 0, 1: the buffers of the two pre-pass
 * streams (batch b of the handle scatters into buffer b mod 2; er_tsdf_reproject into buffer 0), 2: the buffer of the colour calls.  A cell of
 * such a buffer holds (0xFFFF - counter) << 16 | depth; the counter advances once per batch or frame that scatters into the buffer and the
 * buffer is refilled when it would pass 0xFFFF.  epoch <= 0xFFFF is the value the NEXT use advances from. */
int er_tsdf_set_zbuf_epoch(er_tsdf_t h, int which, unsigned epoch);

/* Device depth produced asynchronously: the pre-passes of the NEXT er_tsdf_integrate_frames calls (both internal pre-pass
 * streams) wait for this hipEvent_t (recorded by the caller after the producer of the depth buffer) instead of requiring a
 * synchronised stream.  (Host depth needs no event: it is read by the copy inside the call.) */
int er_tsdf_wait_event(er_tsdf_t h, void* hip_event);

/* Empties the volume (data_.clear()): every unit is released and zero-filled, the hash map is emptied, flags are cleared.
 * Buffers, streams and the unit-shard setting are kept. */
int er_tsdf_reset(er_tsdf_t h);

/* Sticky error flags + the number of depth pixels skipped because their unit index left [0,512) (> +-96 m, where the
 * reference's hash_key would alias another unit).  A POLL: it does not wait for queued batches, so a program can call it
 * after every er_tsdf_integrate_frames and fail fast instead of learning about an exhausted pool in SaveWorld. */
#define ER_STATUS_POOL_EXHAUSTED 1
#define ER_STATUS_TABLE_FULL 2
int er_tsdf_status(er_tsdf_t h, int* flags, long* out_of_range_pixels);

/* data_ map access (TSDFVolume.h:27) as used by SaveWorld. */
int er_tsdf_unit_count(er_tsdf_t h, int* count);
int er_tsdf_unit_keys(er_tsdf_t h, int* keys_host);                  /* ascending hash_key order */
int er_tsdf_read_unit(er_tsdf_t h, int key, float* sdf_host, float* weight_host);  /* 64^3 floats each */

/* Sum of weight_ over the volume = number of voxel updates so far (TSDFVolume.cpp:90,94). */
int er_tsdf_sum_weight(er_tsdf_t h, double* sum);

/* TSDFVolume::SaveWorld's voxel filter (TSDFVolume.cpp:104-132) on device.  Writes (x,y,z,intensity)
 * float4 per point, units in ascending key order, voxels in i,j,k order.  out_host may be NULL to query
 * the count; capacity is in points. */
int er_tsdf_extract_world(er_tsdf_t h, float* out_host, long capacity, long* count);

/* Zero-crossing points of the resident volume (the consumer of world.pcd, kinfu's mesh/point output, does this
 * on the host after reading the file back): for every observed voxel and its +x / +y / +z neighbour (also across unit
 * borders), both with weight != 0 and sdf of strictly opposite sign, the point where the surface crosses the lattice edge,
 * p = voxel position + F / (F - Fn) * voxel size along that axis (metres, float32; position = (float)(global index * 3/512)).
 * float4 per point = x y z axis(0,1,2); units in ascending key order, voxels in i,j,k order, axes x,y,z.
 * out_host may be NULL to query the count; capacity is in points. */
int er_tsdf_extract_surface(er_tsdf_t h, float* out_host, long capacity, long* count);

/* er_tsdf_extract_surface's list with a normal per point: what the kinfu fragment step writes into cloud_bin_<i>.pcd and CCorresApp::LoadData
 * (CorresApp.cpp:82-99) and FragmentOptimizer read back -- replaces a host pass over the whole volume (read every unit back, rebuild a dense
 * grid, take differences there).  The normal is the normalised central difference of the sdf at the point's nearest voxel
 * v = rint((double)p / (3/512)): g_a = S[v + e_a] - S[v - e_a], n = g / sqrt((gx gx + gy gy) + gz gz), float32, every operation rounded on its own.
 * It exists iff v and its six neighbours are observed (weight != 0; voxels of absent or dropped units and outside the 512-unit lattice are not)
 * and the gradient is not zero; it points towards positive sdf = free space.
 * points_host: 4 floats per point (x y z axis), bit-identical to er_tsdf_extract_surface; normals_host: 4 floats per point (nx ny nz 0;
 * NaN NaN NaN 0 where the rule gives none).  Either may be NULL to query the count; capacity is in points. */
int er_tsdf_extract_oriented(er_tsdf_t h, float* points_host, float* normals_host, long capacity, long* count);

/* Marching cubes on the resident volume (the triangle connectivity the pipeline's next step -- kinfu's mesh output,
 * outside the reference repository -- builds from world.pcd).  A cell of 2 x 2 x 2 voxels yields triangles only if all eight are
 * observed (weight != 0); a corner is inside iff sdf < 0; vertices are the linear zero crossings on the lattice edges, in metres.
 * tri_host: 9 floats per triangle (three vertices x, y, z; the normal of the winding points towards positive sdf = free space);
 * order: units by ascending key, cells in i, j, k order, triangles in table order.  Vertices shared by neighbouring cells are
 * bit-identical, so the soup can be welded by exact comparison.  tri_host == NULL: only counts.  er_mc_table copies the 256 x 16
 * case table (three edge ids per triangle, 255-terminated; conventions in csrc/er_mc_table.h) -- host only, no GPU needed. */
int er_tsdf_extract_mesh(er_tsdf_t h, float* tri_host, long capacity_triangles, long* n_triangles);
int er_mc_table(unsigned char out[256 * 16]);

/* The same mesh INDEXED (what kinfu's mesh output hands to a viewer): unique vertices, a normal each, and int32 triangles.
 * Triangles: exactly er_tsdf_extract_mesh's, in its order, as three indices into the vertex list -- verts[tri] reproduces the soup bit for bit.
 * A vertex is a lattice EDGE (its lower voxel L and an axis) that at least one emitted triangle uses: the edge is crossed, (F_L < 0) != (F_H < 0),
 * and at least one of the up to four cells around it has all eight voxels observed.  It is not keyed by its position: two edges that meet in a
 * voxel whose sdf is exactly 0 give the same coordinates and stay two vertices.  Position: er_tsdf_extract_mesh's expression from the edge's
 * lower end.  Order: the unit of L by ascending key, L in i, j, k order, axes x, y, z -- er_tsdf_extract_surface's order but not its set (a
 * surface point needs two observed voxels of strictly opposite sign; a mesh vertex needs a complete cell and counts sdf == 0 as outside).
 * verts_host: 4 floats per vertex (x y z axis), er_tsdf_extract_surface's layout; normals_host: 4 floats per vertex (nx ny nz 0): the rule of
 * er_tsdf_extract_oriented applied to the vertex position, NaN NaN NaN 0 where it gives none; tri_host: 3 ints per triangle.  Any of the three
 * may be NULL; all three NULL: only counts.  Capacities are in vertices and in triangles; one that is too small is refused with the need in the
 * message, after *n_vertices and *n_triangles have been set, and nothing is written.  More than 2^31 - 1 vertices are refused.  An empty
 * volume, or one without a crossing, gives 0 and 0 and succeeds.  No result depends on the order in which workgroups run: the same bytes on
 * every call. */
int er_tsdf_extract_mesh_indexed(er_tsdf_t h, float* verts_host, float* normals_host, long capacity_vertices, int* tri_host,
                                 long capacity_triangles, long* n_vertices, long* n_triangles);

/* Mesh cleaning: the connected components of an indexed mesh, and the mesh without its small ones.  Definitions, for a mesh
 * of nv vertices and nt triangles int32[nt][3]:
 *   - two vertices are connected if one triangle names both; components are the transitive closure;
 *   - a vertex that no triangle names is a component of its own with 0 triangles;
 *   - a triangle that repeats a vertex (a a b) is legal and connects what it names; duplicate triangles count as often as they occur;
 *   - label[v] is the smallest vertex index of v's component, count[v] the number of triangles in v's component, and the number of
 *     components the number of v with label[v] == v;
 *   - the filter, with min_triangles >= 0 and a flag largest_only: a component is kept iff count >= min_triangles and, with largest_only, it
 *     is also the component with the most triangles (a tie goes to the smaller label).  0 and 1 keep everything.  largest_only with a largest
 *     component below min_triangles gives the empty mesh and succeeds;
 *   - the cleaned mesh: kept vertices in their original order, kept triangles in their original order; a triangle is kept iff its vertices
 *     are; an index becomes the number of kept vertices before it; index[i] is the unfiltered index of cleaned vertex i.
 * Every result is defined without reference to any order of execution: the same bytes on every call.
 *
 * er_mesh_components labels any indexed mesh held in host memory on `device`.  label_host [n_vertices], count_host [n_vertices] and rounds
 * (the labelling rounds the call needed, a diagnostic) are nullable.  Refused: a NULL argument, negative sizes, n_vertices > 2^31 - 1, no
 * device, and an index outside [0, n_vertices) -- naming the first offending triangle in triangle order, found before any kernel uses an index
 * as an address, with nothing written.  n_triangles == 0 succeeds, every vertex its own component. */
int er_mesh_components(const int* tri_host, long n_triangles, long n_vertices, int device, int* label_host, long* count_host, long* n_components,
                       int* rounds);

/* er_tsdf_extract_mesh_indexed's mesh filtered as above, without the unfiltered mesh leaving device memory: extraction, labelling, selection
 * and compaction run there and only the cleaned arrays are copied back.  verts_host / normals_host: 4 floats per cleaned vertex in
 * er_tsdf_extract_mesh_indexed's layouts; index_host: its index in the unfiltered mesh; tri_host: 3 ints per kept triangle.  Any output
 * pointer may be NULL; all NULL: only counts, those after filtering.  A capacity that is too small is refused with the need in the message,
 * after the counts (and stats) have been set, and nothing is written.  An empty volume gives 0 and 0.  stats (nullable): components found,
 * components kept, vertices dropped, triangles dropped.  With min_triangles <= 1 and largest_only == 0 the three arrays are
 * er_tsdf_extract_mesh_indexed's bit for bit.  A negative min_triangles is refused. */
int er_tsdf_extract_mesh_cleaned(er_tsdf_t h, long min_triangles, int largest_only, float* verts_host, float* normals_host, int* index_host,
                                 long capacity_vertices, int* tri_host, long capacity_triangles, long* n_vertices, long* n_triangles, long stats[4]);

/* Mesh simplification by vertex clustering (Rossignac-Borrel).  Definitions, for nv vertices as float4 rows (x y z .; the 4th
 * column is ignored), optional normals as float4 rows, optional colours (4 bytes r g b a per vertex), nt triangles int32[nt][3] and a cell
 * (float32, metres):
 *   - cell of a vertex: c_a = floor((double)p_a / (double)cell) per axis; its key (c_x + 2^20) << 42 | (c_y + 2^20) << 21 | (c_z + 2^20);
 *   - a cluster is the set of vertices with one key; its lead is its smallest vertex index;
 *   - position of a cluster: q_a = llrint((double)p_a * 2^20) per member (half to even; the product is exact), S_a the int64 sum of q_a over
 *     the n members, x_a = (float)(((double)S_a / (double)n) * 2^-20), every operation rounded on its own; the 4th column is 0.0f.  The sum
 *     is integer arithmetic: exact and associative;
 *   - normal of a cluster: a member contributes iff its three components are finite and below 4096 in magnitude; N_a the int64 sum of
 *     llrint((double)n_a * 2^20) over the contributing members, g_a = (double)N_a, len = sqrt((g_x g_x + g_y g_y) + g_z g_z) in float64, the
 *     normal (float)(g_a / len); NaN NaN NaN when nobody contributes or len == 0; the 4th column is 0;
 *   - colour of a cluster: over the m members with a != 0 each channel is (2 sum + m) / (2 m) in integer division, a = 255; a cluster
 *     without such a member gets 0 0 0 0 (er_tsdf_sample_colors' rounding);
 *   - triangles: (a, b, c) becomes (A, B, C), the clusters of its vertices; it is degenerate, and dropped, iff two of them are equal; two
 *     non-degenerate triangles are duplicates iff one triple is a rotation of the other (the same vertices and the same winding), and of a
 *     set of duplicates the one with the lowest input index stays; opposite windings are not duplicates, both stay; a kept triangle keeps
 *     its own rotation and its place in the input order;
 *   - vertices: a cluster becomes an output vertex iff a kept triangle names it; output vertices are ordered by lead, ascending; a triangle's
 *     indices are the ranks of its clusters in that order;
 *   - side outputs: cluster[v] the output index of v's cluster or -1; members[i] the number of members of the cluster behind output vertex i;
 *     tri_index[j] the input index of kept triangle j; stats: occupied cells, degenerate triangles dropped, duplicates dropped, cells dropped
 *     because no kept triangle names them.
 * Every result is defined without reference to any order of execution: the same bytes on every call.  probes (nullable) is a diagnostic
 * outside that promise: the longest probe sequence of the call in the vertex table and in the triangle table, which depends on arrival order.
 *
 * Refused, each before any kernel uses an index as an address, with nothing written, the message naming the FIRST offender in input order
 * (vertices before triangles): a NULL required argument (the two counts; the vertices and the triangles where there are any; an output of
 * normals or colours without its input) or negative sizes; n_vertices or n_triangles > 2^31 - 1; no device; a cell that is not finite or
 * is <= 0; a coordinate that is not finite or is >= 4096 m in magnitude ("vertex <v> ..."); a c_a outside [-2^20, 2^20) ("vertex <v> ...");
 * a triangle index outside [0, n_vertices) ("triangle <t> names vertex <i>, outside [0, <nv>)"); a capacity that is too small, refused after
 * the counts, stats and probes have been set.  n_vertices == 0 or n_triangles == 0 gives the empty mesh and succeeds: counts and stats 0,
 * cluster all -1, and no vertex is looked at.
 *
 * er_mesh_simplify clusters any indexed mesh held in host memory on `device`.  Every output pointer is nullable (verts_out, normals_out:
 * 4 floats per output vertex; colors_out: 4 bytes; members_out: int32; tri_out: 3 ints per kept triangle; tri_index_out: int32 per kept
 * triangle; cluster_out: int32 [n_vertices]); with all of them NULL the call returns only counts and stats.  Capacities are in output
 * vertices and kept triangles. */
int er_mesh_simplify(const float* verts_host, const float* normals_host, const uint8_t* colors_host, long n_vertices, const int* tri_host,
                     long n_triangles, float cell, int device, float* verts_out, float* normals_out, uint8_t* colors_out, int* members_out,
                     long capacity_vertices, int* tri_out, int* tri_index_out, long capacity_triangles, int* cluster_out, long* n_vertices_out,
                     long* n_triangles_out, long stats[4], long probes[2]);

/* The simplified mesh of the resident volume, without the unsimplified mesh leaving device memory: er_tsdf_extract_mesh_indexed's mesh --
 * er_tsdf_extract_mesh_cleaned's, with its semantics on the UNSIMPLIFIED mesh, if min_triangles > 1 || largest_only -- is clustered as
 * above where it lies and only the simplified arrays are copied back.  want_colors: the unsimplified vertices are coloured on the device
 * (er_tsdf_sample_colors' rule) and averaged per cluster; it is refused before er_tsdf_color_enable, and colors_host without it is refused.
 * Output layouts, nullable pointers, capacities, stats and probes as for er_mesh_simplify; before (nullable): vertices and triangles of the
 * mesh that was clustered.  An empty volume, or a cleaning that keeps nothing, gives 0 and 0.  A negative min_triangles is refused. */
int er_tsdf_extract_mesh_simplified(er_tsdf_t h, float cell, long min_triangles, int largest_only, int want_colors, float* verts_host,
                                    float* normals_host, uint8_t* colors_host, int* members_host, long capacity_vertices, int* tri_host,
                                    long capacity_triangles, long* n_vertices, long* n_triangles, long stats[4], long before[2], long probes[2]);

/* Mesh smoothing (Taubin lambda|mu) and vertex normals from the triangles.  Definitions, for nv vertices as float4 rows
 * (x y z .; the 4th column is ignored), nt triangles int32[nt][3], iterations, lambda and mu (float32) and a flag fix_boundary.  All
 * arithmetic is float64 or int64, never fused, every operation rounded on its own:
 *   - edges: triangle t and corner c give the unordered pair {tri[t][c], tri[t][(c + 1) % 3]}; a pair whose two entries are equal is skipped.
 *     The multiplicity of an edge is the number of (t, c) that give it.  N(v) is the SET of w with {v, w} an edge and deg(v) = |N(v)|: a
 *     duplicated triangle, or two triangles on one edge, give that neighbour once.  A boundary edge has multiplicity 1, a boundary vertex is
 *     an end of one, a non-manifold edge has multiplicity >= 3;
 *   - a pass with factor f: a vertex with deg == 0 keeps its position bits and, with fix_boundary, so does every boundary vertex.  Every other
 *     vertex moves, per axis: S_a the int64 sum over w in N(v) of llrint((double)p_w,a * 2^20) (half to even), m_a = ((double)S_a /
 *     (double)deg) * 2^-20, x'_a = (float)((double)p_a + (double)f * (m_a - (double)p_a)).  All vertices read the positions the pass started
 *     with.  A pass whose factor is exactly 0 is not run;
 *   - an iteration is a pass with lambda, then a pass with mu; pass 2 i is iteration i's first, pass 2 i + 1 its second, run or not.  mu = 0 is
 *     plain Laplacian smoothing;
 *   - the output position has 0.0f in its 4th column; with iterations == 0 it is the input's bits, 4th column 0;
 *   - range guard: after every pass every coordinate has to be finite and below 4096 m in magnitude (a negative mu extrapolates); otherwise the
 *     call is refused with nothing written, naming the smallest such pass and in it the smallest vertex;
 *   - normals, from the OUTPUT positions: per triangle (a, b, c), d1 = (double)p_b - (double)p_a, d2 = (double)p_c - (double)p_a per
 *     component, cross_x = d1_y d2_z - d1_z d2_y and cyclic (each product rounded before the subtraction), k_a = llrint(cross_a * 2^32).  k is
 *     added once per corner to that corner's vertex sum N_a; the sums are uint64 in two's complement, so wrapping is the definition.  Then
 *     g = (double)(int64)N, len = sqrt((g_x g_x + g_y g_y) + g_z g_z), the normal (float)(g_a / len); NaN NaN NaN iff len == 0, which covers
 *     a vertex no triangle names; the 4th column is 0;
 *   - side outputs: degree[v] int32; boundary[v] uint8 (1 or 0, whether or not fix_boundary is set); stats: distinct edges, boundary edges,
 *     non-manifold edges, vertices that no pass moves (deg == 0, and with fix_boundary the boundary vertices).
 * Every result is defined without reference to any order of execution: the same bytes on every call.  probes (nullable) is a diagnostic
 * outside that promise: the longest probe sequence of the call in the edge table.
 *
 * Refused, each before any kernel uses an index as an address, with nothing written, the message naming the FIRST offender in input order
 * (vertices before triangles): a NULL required argument (the vertices and the triangles where there are any) or negative sizes; n_vertices
 * > 2^31 - 1 or 3 n_triangles > 2^31 - 1 (int32 edge instances); no device; iterations outside [0, 1024]; lambda or mu not finite or above
 * 1 in magnitude; a coordinate that is not finite or is >= 4096 m in magnitude ("vertex <v> ..."); a triangle index outside [0, n_vertices)
 * ("triangle <t> names vertex <i>, outside [0, <nv>)").  n_vertices == 0 succeeds with no array written (stats 0); n_triangles == 0
 * succeeds: the positions pass through, normals NaN, degrees 0.
 *
 * er_mesh_smooth smooths any indexed mesh held in host memory on `device`.  Every output pointer is nullable (verts_out, normals_out: 4 floats
 * per vertex; degree_out: int32, boundary_out: uint8 [n_vertices]).  iterations == 0 with normals_out is the library's "vertex normals from
 * triangles" call. */
int er_mesh_smooth(const float* verts_host, long n_vertices, const int* tri_host, long n_triangles, int iterations, float lambda, float mu,
                   int fix_boundary, int device, float* verts_out, float* normals_out, int* degree_out, uint8_t* boundary_out, long stats[4],
                   long probes[1]);

/* The smoothed mesh of the resident volume, without an intermediate mesh leaving device memory.  Stages: er_tsdf_extract_mesh_indexed's mesh;
 * er_tsdf_extract_mesh_cleaned's filter if min_triangles > 1 || largest_only; the smoothing above; er_mesh_simplify's clustering if cell > 0
 * (cell == 0 is legal here and skips it; a negative or non-finite cell is refused).  want_colors: the vertices are coloured at their
 * UNSMOOTHED positions -- the voxels the surface was observed in -- by er_tsdf_sample_colors' rule and the colours travel unchanged by vertex
 * index (the clustering then averages them); refused before er_tsdf_color_enable, and colors_host without it is refused.  The normals are
 * the triangle normals of the smoothed mesh (the clustering then combines them by its own rule).  With iterations == 0 the smoothing stage is
 * skipped entirely and the arrays are the existing routes' bit for bit (the 4th column of a vertex and the TSDF-gradient normals included).
 * Refusals are those of the stages that run.  Counts first: *n_vertices and *n_triangles are set, then a capacity that is too small is
 * refused with nothing written.  smooth_stats, simplify_stats (as the two calls above; zero for a stage that did not run) and before
 * (vertices and triangles of the mesh that was smoothed) are nullable.  An empty volume gives 0 and 0.  Without the clustering the counts
 * are those of the mesh that is smoothed: a call with every output and smooth_stats NULL returns them without smoothing. */
int er_tsdf_extract_mesh_smoothed(er_tsdf_t h, int iterations, float lambda, float mu, int fix_boundary, float cell, long min_triangles,
                                  int largest_only, int want_colors, float* verts_host, float* normals_host, uint8_t* colors_host,
                                  long capacity_vertices, int* tri_host, long capacity_triangles, long* n_vertices, long* n_triangles,
                                  long smooth_stats[4], long simplify_stats[4], long before[2]);

/* TSDFVolume::SaveWorld's inverse: a world.pcd voxel list back into a volume.  xyzi_host: n rows x y z intensity in er_tsdf_extract_world's
 * layout -- x, y, z integer voxel indices as floats, i + (xi - 256) * 64; intensity = the sdf.  Afterwards every listed voxel is (intensity, 1)
 * and every other voxel of a created unit (+0, 0); the created units are those with at least one listed voxel, *n_units (nullable) their number.
 * world.pcd carries no weights: 1 only marks "observed", so the volume is one to extract from, not one to go on integrating into.  What
 * SaveWorld's filter dropped (|sdf| >= 0.98, never-observed voxels) stays unobserved.
 * Refused, each naming the first offending row: a coordinate that is not an integer value or lies outside the 512-unit lattice; a NaN
 * intensity; a voxel listed twice.  Also refused: a volume that already holds units (er_tsdf_reset it first), and a list that needs more than
 * max_units units (the message names both numbers).  After any of these refusals the volume is empty -- also the one that held units.
 * n == 0 succeeds with no units. */
int er_tsdf_import_world(er_tsdf_t h, const float* xyzi_host, long n, int* n_units);

/* Colour: registered RGB frames splatted into per-voxel integer accumulators, and the colour of a point read back from them.
 * The reference has no colour code: these entries restate tests/color_restatement.py bit for bit.  Everything is integer arithmetic on sums of
 * bytes, so the accumulators hold the same bits whatever the batch split, the frame order, the stream or the run.
 *
 * er_tsdf_color_enable allocates and zero-fills max_units x 64^3 records of uint32 r_sum, g_sum, b_sum, n (16 bytes a voxel, 4 MiB a unit), indexed
 * by the unit's pool slot, voxel (i * 64 + j) * 64 + k as the sdf.  Idempotent.  A failed allocation is a refusal that names the bytes.  A volume
 * that never enables colour allocates nothing and behaves as before.  er_tsdf_reset zeroes the accumulators, er_tsdf_drop_units those of the
 * dropped units.  Band, raw and weighted export / import do not carry colour, and every colour entry is refused while er_tsdf_set_unit_shard
 * has world > 1.  A record is added to as two 64-bit words (r | g << 32), (b | n << 32): below 2^24 samples per voxel no field carries into its
 * neighbour; beyond that the sums are wrong and nothing checks it.
 * All other colour entries are refused before er_tsdf_color_enable. */
int er_tsdf_color_enable(er_tsdf_t h);

/* The 64^3 x 4 accumulator words of one EXISTING unit to / from host memory; a key without a unit is refused. */
int er_tsdf_read_unit_color(er_tsdf_t h, int key, uint32_t* rgbn_host);
int er_tsdf_write_unit_color(er_tsdf_t h, int key, const uint32_t* rgbn_host);

/* The splat.  depth: n x rows x cols uint16; rgb: n x rows x cols x 3 bytes, registered to the depth image and of its size; both in host memory or
 * (on_device != 0) both complete in device memory; T: er_tsdf_integrate_frames' poses of the same frames.  The frames are meant to have been
 * integrated already, so that their units exist; nothing enforces it.  Pixel (u, v) of a frame contributes iff
 *   1. d = depth != 0, and
 *   2. scale_depth(d, u, v) > 0.001f: the pixels TSDFVolume::IntegrateVolumeUnit uses (TSDFVolume.cpp:29, 82; beyond integration_trunc it is 0);
 *   3. its world point -- TSDFVolume::UVD2XYZ, then ((T0 x + T1 y) + T2 z) + T3 in float64, the chain behind the unit keys -- gives the voxel
 *      g_a = floor(p_a / unit length + 0.5) per axis; a g_a outside [-16384, 16384) sends the pixel to out_of_range;
 *   4. the unit (g_a + 16384) / 64 exists; otherwise the pixel goes to no_unit;
 *   5. then (r, g, b, 1) is added to voxel (g_a + 16384) & 63 of that unit.
 * stats (nullable): pixels added, no_unit, out_of_range, of this call.  n == 0 succeeds.  Two calls accumulate.  The call runs on the handle's
 * stream behind the voxel passes and returns when the device work is done.
 * warp (nullable): er_tsdf_integrate_frames' warp of the same frames.  Depth and colour are first warped into the frame's virtual camera -- per
 * frame (Z, C') of er_tsdf_reproject_color below -- and steps 1 to 5 then run on (Z, C'); after that everything is rigid. */
int er_tsdf_color_frames(er_tsdf_t h, int n, const uint16_t* depth, const uint8_t* rgb, int on_device, const double* T, const er_warp* warp,
                         long stats[3]);

/* er_tsdf_reproject with the colour image, for ONE frame in place on host memory (colour need not be enabled).  Afterwards depth holds Z, exactly
 * what er_tsdf_reproject returns, and rgb holds C': C'[c] = C[winner(c)] where winner(c) is the LOWEST source pixel index p with depth[p] != 0
 * whose reprojection succeeds with cell c and a 16-bit depth equal to Z[c] != 0; 0 0 0 where Z[c] == 0.  The rule is a definition and does not
 * depend on any order: where the reference's replay of zero-depth writes would have erased an equal-depth earlier write, the colour may come
 * from that pixel. */
int er_tsdf_reproject_color(er_tsdf_t h, uint16_t* depth_inout_host, uint8_t* rgb_inout_host, const float* ctr_host, int resolution, float length,
                            const double seg[16], const double madj[16]);

/* Colour at n points of host memory, 4 floats per row (x y z in metres, the 4th ignored: er_tsdf_extract_surface's, er_tsdf_extract_oriented's and
 * er_tsdf_extract_mesh_indexed's vertex layout) -> rgba_host, 4 bytes per point.  v = rint((double)p / unit length) per component, half to even
 * (er_tsdf_extract_oriented's nearest voxel).  Level 0: voxel v, if its unit exists and its n > 0.  Level 1 otherwise: the 64-bit sums over the
 * 27 voxels v + {-1, 0, 1}^3 that lie on the lattice in existing units, across unit borders.  Channel = (2 sum + n) / (2 n) in integer division
 * (round half up), a = 255.  No sample, a non-finite coordinate or a v off the lattice gives 0 0 0 0.  counts (nullable): points coloured at
 * level 0 and at level 1. */
int er_tsdf_sample_colors(er_tsdf_t h, const float* points_host, long n, uint8_t* rgba_host, long counts[2]);

/* The resident volume ray-cast from a pose: the model side of frame-to-model tracking (er_odom_align_model below) and a
 * direct picture of what er_tsdf_integrate_frames built.  The reference tree has no ray caster (KinFu's lives in the author's PCL fork):
 * this entry restates tests/raycast_restatement.py, the numpy statement of csrc/er_raycast_math.h, bit for bit, and NOTHING here is checked
 * against PCL.  Per pixel (u, v) of a cols x rows image with cam4 = (fx, fy, cx, cy) -- independent of the volume's integration image -- the
 * ray through the pixel from world_T_camera T (row-major float64, cast once to float32) is sampled at t_k = t_min + k step, k = 0 ..
 * ceil((t_max - t_min) / step) - 1, at the nearest voxel; a sample is observed iff its unit exists, is not dropped and its weight is not 0.
 * Two successive observed samples with sdf >= 0 then < 0 are a hit, with < 0 then >= 0 the ray ends without one.  The crossing is refined
 * on trilinear values (all eight corners observed, else on the two nearest-voxel values); the normal is the negated, normalised central
 * difference of the trilinear sdf one voxel to either side of the hit point, rotated into the camera frame (NaN where one of the six
 * values is missing: the vertex stays).
 * rec_out (nullable): er_odom's record map, cols * rows * 2 float4 = {vertex, 0}, {normal, 0} in the CAMERA frame, NaN where there is no
 * hit; depth_out (nullable): cols * rows uint16 = rint(1000 vertex.z), 0 where there is none or it leaves 1 .. 65535.  Both in host
 * memory, or both in device memory of the handle's device when out_on_device.  params NULL = the defaults.  Refused: cols or rows <= 0,
 * a t_min, t_max or step that is not finite, step <= 0, more than 65536 steps, both outputs NULL; t_max <= t_min gives an empty image.
 * Runs on the handle's stream behind every queued batch, like the er_tsdf_extract_* calls, and returns when the outputs are complete. */
typedef struct er_raycast_params {
  float t_min, t_max, step;   /* metres along the normalised ray: (0.0, 4.0, 0.8 * 0.03) */
} er_raycast_params;
int er_raycast_params_default(er_raycast_params* p);
int er_tsdf_raycast(er_tsdf_t h, int cols, int rows, const float cam4[4], const double T[16], const er_raycast_params* params,
                    void* rec_out /* cols*rows*2 float4, nullable */, uint16_t* depth_out /* nullable */, int out_on_device);

/* A LIST of ray-casts in one launch: job j casts volume vol[j] into a cols[j] x rows[j] image with cam4[4 j ..] from the pose
 * T[16 j ..] under params[j] (params NULL: the defaults for every job), exactly as er_tsdf_raycast does -- the same bits, whatever else is in
 * the list.  The same volume may appear in any number of jobs; all volumes must live on ONE device.  Outputs are DEVICE memory only:
 * rec_out_dev[j] (nullable) and depth_out_dev[j] (nullable; the whole array may be NULL), not both NULL.  The launch goes on a stream of the
 * call's own, behind every queued batch of every volume named, and the call returns when all outputs are complete.  Everything er_tsdf_raycast
 * refuses is refused for the whole list before anything is launched, the message naming the job ("job 3: ..."); also more than 65535 jobs and
 * volumes of two devices.  n_jobs == 0 returns 0 and touches nothing. */
int er_tsdf_raycast_batch(int n_jobs, const er_tsdf_t* vol, const int* cols, const int* rows, const float* cam4 /* [n_jobs][4] */,
                          const double* T /* [n_jobs][16] */, const er_raycast_params* params /* [n_jobs], nullable */,
                          void* const* rec_out_dev, uint16_t* const* depth_out_dev);

/* Multi-GPU frame split: for the given key list write sum-ready planes into dev_buf
 * (n_keys * 2 * 64^3 floats: [key][0] = sdf*weight, [key][1] = weight; zeros for keys absent here), and
 * after an external all-reduce(sum) read them back as weight = W, sdf = SW / W. */
int er_tsdf_export_weighted(er_tsdf_t h, const int* keys_host, int n_keys, float* dev_buf);
int er_tsdf_import_weighted(er_tsdf_t h, const int* keys_host, int n_keys, const float* dev_buf);
/* The same layout with [key][0] = sdf itself: a unit BIT FOR BIT -- how a unit that only one GPU touched travels (TSDFVolume.cpp:93-94 is a
 * sum only where frames of two GPUs met; sdf * w / w would round the others for nothing).  import_raw creates the unit if it is absent and
 * overwrites it otherwise. */
int er_tsdf_export_raw(er_tsdf_t h, const int* keys_host, int n_keys, float* dev_buf);
int er_tsdf_import_raw(er_tsdf_t h, const int* keys_host, int n_keys, const float* dev_buf);
/* Round 6, BAND RECORDS: a unit as its observed voxels only (weight_ != 0: the truncation band and the free space in front of it, about a quarter of a
 * touched unit), the sdf_ only where it is not exactly 1 (free space: four observed voxels out of five) and the weight_ as 16 bits when every weight of
 * the unit is a frame count below 65536.  A never-updated voxel is (+0, 0) (TSDFVolumeUnit.cpp:4-21), so a record restores a unit bit for bit.
 * Records are DEVICE memory, 8-byte aligned, a whole number of 32-bit words (layout: csrc/er_tsdf_band.hip, "band records").  band_sizes: the record size in
 * words of each unit this GPU holds (a key it does not hold is an error).  export_band: the records of the given units back to back into dev_block
 * (sizes as band_sizes returned them; a volume that changed in between is an error).  merge_band: the OWNER's step of the frame-split merge -- unit
 * keys[u] becomes the sum of its own voxels and nsrc[u] <= 16 records (recs[16 u + k], the other GPUs' in rank order; self_pos[u] of them come before
 * its own voxels in that order): SW = sum fl(sdf_r w_r), W = sum w_r, sdf = SW / W, TSDFVolume.cpp:93-94 as a sum in an order fixed by the arguments.
 * import_band: create / overwrite units from records.  drop_units: this GPU hands the units over -- they are zeroed and disappear from
 * er_tsdf_unit_count / unit_keys / read_unit / band_sizes / the extractions.  An import (raw, weighted or band) brings back the units it names.  The
 * next er_tsdf_integrate_frames call with at least one frame brings back ALL of them, whichever units its frames touch: the touched ones hold those
 * frames alone, the others are allocated, never-updated units (all voxels (+0, 0), as far units are after any integration), and the next merge counts
 * this GPU among their holders with an empty record.  All of them run on the handle's stream and return when the device work is done. */
int er_tsdf_band_sizes(er_tsdf_t h, const int* keys_host, int n_keys, int* words_host);
int er_tsdf_export_band(er_tsdf_t h, const int* keys_host, const int* words_host, int n_keys, void* dev_block);
int er_tsdf_merge_band(er_tsdf_t h, const int* keys_host, int n_keys, const int* nsrc, const int* self_pos, const void* const* recs);
int er_tsdf_import_band(er_tsdf_t h, const int* keys_host, int n_keys, const void* const* recs);
int er_tsdf_drop_units(er_tsdf_t h, const int* keys_host, int n_keys);

/* Multi-GPU, the bit-exact alternative: shard the volume BY UNIT.  Every GPU is fed ALL frames and runs
 * their pre-pass, but only allocates / integrates / reports the units with er_unit_owner(key, world) == rank.  Units are disjoint
 * (TSDFVolume.cpp:45-63) and each still sees every frame in order, so the union of the GPUs' volumes equals the single-GPU
 * volume bit for bit and no collective touches the volume.  Must be set before the first frame. */
int er_tsdf_set_unit_shard(er_tsdf_t h, int rank, int world);
int er_unit_owner(int key, int world);          /* (xi + yi + zi) mod world: diagonal stripes of the unit lattice */

/* Multi-GPU frame split behind the C ABI (the Python path over torch.distributed is parallel.py).  One
 * communicator per GPU over RCCL (xGMI inside a node; librccl is loaded on first use):
 *   er_comm_unique_id + er_comm_create   one PROCESS per GPU: rank 0 draws the 128-byte id and hands it to the other ranks
 *                                        out of band (a file, a socket, torch.distributed), then every rank creates its
 *                                        communicator (ncclCommInitRank; collective: all ranks must call it);
 *   er_comm_create_local                 ONE process, n GPUs, one host thread per GPU afterwards (ncclCommInitAll).
 * er_tsdf_allreduce merges the private volumes of the ranks after each integrated its own contiguous frame block
 * (er_frame_block).  Every rank calls it once.  It is the OWNER MERGE (round 6; csrc/er_merge_protocol.h: merge_protocol_owner), a
 * reduce-scatter by volume unit:
 *   agree on the key count; all-gather the touched unit keys with their observed-voxel counts -- every rank then knows who touched what and how
 *   much; every unit of the union gets an OWNER, the toucher that observed most of it; every other toucher sends the owner a band record of
 *   its voxels (above) in ONE grouped ncclSend / ncclRecv step -- each (sender, owner) pair is an xGMI link of its own --; the owner adds the
 *   records to its own voxels IN RANK ORDER in one kernel: weights exact, sdf within 1e-5 of the sequential running mean of TSDFVolume.cpp:93-94
 *   (the float32 summation order differs from the frame order), and bit-reproducible: the order is a function of the key sets, not of the wire;
 *   the non-owners drop their copies.
 * root == ER_MERGE_DISTRIBUTED stops there: the merged volume stays distributed, every unit complete on exactly one rank (SaveWorld is per unit,
 * TSDFVolume.cpp:104-132: bin/Integrate --gpus N concatenates the ranks' extractions by key).  root >= 0: the owners then send their finished
 * units, as band records, to `root` in a second grouped step; root == ER_MERGE_ALL (-1): to every other rank.  Units only ONE rank touched are
 * that rank's: they stay where they are (distributed) or travel bit for bit (records restore a unit exactly).
 * A communicator of more than 17 ranks is refused (an owner adds the records of at most 16 other touchers).  Round 5's ring reduction of whole
 * planes is gone; ER_MERGE_IMPL, which selected it, is no longer read.
 * union_units (nullable) receives the size of the key union; er_comm_merge_stats what the last merge of this communicator moved: stats[0] union,
 * [1] multi-toucher units, [2] single-toucher units, [3] units this rank handed over, [4] units this rank summed, [5] bytes handed to a
 * reduction collective (always 0: the slot of round 5's ring reduction), [6] bytes this rank sent, [7] bytes received.  er_comm_merge_stats_owner:
 * [0] protocol of the last merge (always 1, the owner merge), [1] union, [2] multi-toucher, [3] single-toucher, [4] units this rank owns afterwards, [5] of
 * which it summed, [6] units it handed over, [7] / [8] bytes sent / received in the step to the owners, [9] / [10] in the step to the root /
 * everybody, [11] bytes round 5's ring reduction would have been handed for the same key sets (2 MiB per multi-toucher unit). */
typedef struct er_comm_s* er_comm_t;
#define ER_COMM_ID_BYTES 128
int er_comm_unique_id(unsigned char id[ER_COMM_ID_BYTES]);
int er_comm_create(const unsigned char id[ER_COMM_ID_BYTES], int rank, int world, int device, er_comm_t* out);
int er_comm_create_local(int n, const int* devices, er_comm_t* out /* n handles */);
/* n <= 16 ranks = n host threads of this process, ALL on one device, no RCCL: the same merge protocol over the same device volumes and
 * band-record kernels, the point-to-point steps as device-to-device copies.  For boxes with one GPU (RCCL refuses two ranks on one device): `Integrate --gpus N --same_device`, tests. */
int er_comm_create_loopback(int n, int device, er_comm_t* out /* n handles */);
int er_comm_destroy(er_comm_t c);
int er_comm_rank(er_comm_t c);
int er_comm_world(er_comm_t c);
#define ER_MERGE_ALL (-1)
#define ER_MERGE_DISTRIBUTED (-2)
int er_tsdf_allreduce(er_tsdf_t h, er_comm_t c, int root, int* union_units);
int er_comm_merge_stats(er_comm_t c, long long stats[8]);
int er_comm_merge_stats_owner(er_comm_t c, long long stats[12]);
/* Contiguous frame block [lo, hi) of `rank` (IntegrateApp.cpp:190-226 is the loop being split). */
void er_frame_block(int n_frames, int rank, int world, int* lo, int* hi);

/* Kernel timing: HIP events on the handle's stream around every `enable`-th IntegrateVolumeUnit launch (1 = every launch, 0 = off;
 * each timed launch puts two more packets on the stream, about 2 % of the frame rate when every launch is timed).  get_profile
 * returns the sum and the number of the TIMED launches, all frames and all unit visits since set_profiling. */
int er_tsdf_set_profiling(er_tsdf_t h, int enable);
int er_tsdf_get_profile(er_tsdf_t h, double* integrate_ms_total, long* integrate_launches, long* frames,
                        long* unit_visits);

/* Timeline of the batch pipeline (scripts/slow_mode_probe.py).  While on, every batch of er_tsdf_integrate_frames records the host's monotonic
 * clock at three points and seven timing events on its two streams; off (the default) no event is created or recorded.  Switching on waits
 * for the handle's streams, drops what an earlier recording left and records the base event every time is measured against; switching off only
 * stops the recording, also with batches in flight: what was recorded stays readable.
 * er_tsdf_get_timeline waits for the recorded batches and returns one row per batch, in order.  meta: ER_TIMELINE_META long long per row --
 * batch number (it restarts at er_tsdf_reset), pipeline slot, pre-pass stream, frames.  times_ms: ER_TIMELINE_TIMES doubles per row, all in
 * ms since the hook was switched on --
 *   0..2  host: entry of the batch, behind the wait for the slot's page-locked constants block, return;
 *   3..7  pre-pass stream: behind the wait for the slot's last voxel pass, behind the constants copy, behind k_reproject_fix (without a warp
 *         nothing runs there: the stream as it stands), behind k_prepare, behind k_plan;
 *   8, 9  voxel stream: in front of and behind k_integrate.
 * With meta or times_ms NULL only *n_rows is set (the rows recorded so far; nothing is waited for).  Otherwise the first min(cap, rows) rows
 * are written, *n_rows is their number and the record is CLEARED. */
#define ER_TIMELINE_META 4
#define ER_TIMELINE_TIMES 10
int er_tsdf_set_timeline(er_tsdf_t h, int on);
int er_tsdf_get_timeline(er_tsdf_t h, int cap, long long* meta, double* times_ms, int* n_rows);

/* ------------------------------------------------------------- path B: ICP ---- */
typedef struct er_cloud_s* er_cloud_t;

/* pointclouds_[i] after the NaN-normal filter (CorresApp.cpp:94-98): n points, xyz and normals as
 * separate float[3*n] host arrays (AoS xyz xyz ...).  grid_cell = edge of the uniform search grid
 * built over this cloud when it is used as a TARGET; must be >= every max distance queried later
 * (use reg_dist_, CorresApp.cpp:16).  n < 2^27 (134 217 728) points: the search kernels address a cloud with 32-bit byte offsets; larger
 * clouds are refused. */
int er_cloud_create(const float* xyz_host, const float* normal_host, int n, float grid_cell, int device,
                    er_cloud_t* out);
/* The clouds of a LIST of fragments in one call (LoadData's loop, CorresApp.cpp:82-110): xyz_host[i] / normal_host[i] hold counts[i] points.
 * All uploads are queued up front (coordinates and normals on two copy streams); chunks of up to 8 clouds share their device allocations
 * and ONE set of grid launches, built while the later chunks are still uploading; the host waits once per chunk.  Page-locked input
 * arrays (er_host_alloc) make the uploads asynchronous: the list is then bound by PCIe (6 x 4 bytes per point), not by the host.
 * All or nothing: on failure no cloud is left behind.  out[i] as er_cloud_create; the clouds may be destroyed in any order (a chunk's
 * allocations go with its last cloud). */
int er_cloud_create_batch(int n_clouds, const float* const* xyz_host, const float* const* normal_host, const int* counts, float grid_cell,
                          int device, er_cloud_t* out);
/* pointclouds_[i] (CorresApp.cpp:82-99) made from the resident volume without leaving the device: er_tsdf_extract_oriented's list, minus the
 * rows with a NaN normal (CorresApp.cpp:93-98), and, if cube_length > 0, minus the points outside 0 <= x, y, z < cube_length (float32
 * compares; PointCloud::GetCoordinate's cube, far face excluded).  Order kept (a stable compaction on the device).  The cloud lives on the
 * volume's device and equals, in every later result, the one er_cloud_create builds from the same rows taken through host memory.
 * n_points may be NULL.  The call waits for the volume's stream (er_tsdf_set_stream) before the cloud builder's streams read the rows. */
int er_cloud_create_from_tsdf(er_tsdf_t h, float cube_length, float grid_cell, er_cloud_t* out, int* n_points);
int er_cloud_destroy(er_cloud_t c);
int er_cloud_size(er_cloud_t c);

/* Registration pre-check (CorresApp.cpp:249-264): cnt = #{k : NN sqdist(T*src[k], tgt) < max_dist^2}. */
int er_icp_count_inliers(er_cloud_t src, er_cloud_t tgt, const double T[16], double max_dist, int* count);

/* pcl::IterativeClosestPoint::align with TransformationEstimationPointToPlaneLLS as configured at
 * CorresApp.cpp:295-306 (source = src, target = tgt).  guess/out are ROW-MAJOR FLOAT 4x4.
 * stop_rule: 0 = PCL 1.7 DefaultConvergenceCriteria, 1 = PCL <= 1.6 rule.
 * fitness (may be NULL) = mean squared NN distance within max_dist after the final transform. */
int er_icp_align(er_cloud_t src, er_cloud_t tgt, const float guess[16], double max_dist, int max_iter,
                 double transformation_epsilon, int stop_rule, float out[16], int* iterations, int* converged,
                 double* fitness);

/* FindCorrespondence (CorresApp.cpp:144-161, 186-208): pairs (tgt_index, src_index) ascending in
 * src_index, for NN sqdist < dist^2 and normal dot > normal_cos; info36 (nullable) = row-major 6x6
 * information matrix over the untransformed source points. pairs_host holds 2*capacity ints -- pageable host memory,
 * page-locked host memory (er_host_alloc: no staging pass) or, since round 5, DEVICE memory of the clouds' GPU (er_device_alloc:
 * the list stays in HBM, a device-to-device copy of exactly the list; the same holds for every pairs_host of the *_batch forms). */
int er_find_correspondence(er_cloud_t src, er_cloud_t tgt, const double T[16], double dist, double normal_cos,
                           int* pairs_host, int capacity, int* n_pairs, double* info36);

/* The reference runs its two loops over the pair list with "#pragma omp parallel for" (CorresApp.cpp:121,220).
 * The *_batch forms take the whole list of one loop: n pairs (src[i], tgt[i]) on ONE device, per-pair inputs and
 * outputs as arrays (T: n*16 doubles, guess/out: n*16 floats, info36: n*36 doubles, ...).  Results are those of n single
 * calls, bit for bit: integers (counts, iteration counts, correspondence lists) and -- since round 6 -- every float of every transform.  The 29
 * float64 sums of an ICP iteration are added per wave of 64 consecutive points (a function of the pair alone) and from there on as 64-bit fixed-point
 * integers whose power-of-two scales come from certain bounds of the data, so the totals do not depend on how the library groups the work: not on the
 * list a pair is part of, its position, ER_ICP_GROUP or the shares of er_registration_batch (rounds 4-5: they did, in the last bits).
 * Internally a whole group of pairs runs through every stage in one launch; the ICP loop's solve and stop rule stay on the device.
 * The single-pair functions above are the n == 1 case of these.  Clouds are immutable: any number of host threads
 * may use the same cloud concurrently (each call borrows its workspaces from a per-device pool). */
/* Test hook (tests/test_icp_shapes_gpu.py): er_icp_align for one pair with ONE iteration per host visit -- the same kernels, solve and stop rule
 * -- and what every iteration computed.  pts = slices of 256 source points per workgroup, 1..2 (the library's own choice depends on the size of
 * the list); anything else is refused.  Row r (r < row_capacity; *n_rows = rows the loop produced, which may exceed the capacity) holds, after
 * iteration r's decision: totals[29 r ..] the 29 sums exactly as the decision received them (0..20 upper triangle of A^T A row by row, 21..26
 * A^T b, 27 sum of squared distances, 28 correspondence count), fin / delta [16 r ..] the accumulated transform and the last increment,
 * state[3 r ..] = {iterations so far, done, converged}, prev_mse[r].  fx_scale[29] (nullable): the pair's fixed-point scales.  out, iterations,
 * converged as er_icp_align returns them, bit for bit. */
int er_icp_align_trace(er_cloud_t src, er_cloud_t tgt, const float guess[16], double max_dist, int max_iter, double transformation_epsilon,
                       int stop_rule, int pts, int row_capacity, double* totals, float* fin, float* delta, int* state, double* prev_mse,
                       double* fx_scale, int* n_rows, float out[16], int* iterations, int* converged);

int er_icp_count_inliers_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T, double max_dist, int* counts);
int er_icp_align_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const float* guess, double max_dist, int max_iter,
                       double transformation_epsilon, int stop_rule, float* out, int* iterations, int* converged,
                       double* fitness);
int er_find_correspondence_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T, double dist,
                                 double normal_cos, int* const* pairs_host, const int* capacity, int* n_pairs,
                                 double* info36);

/* SURVEY.md 8f-3, first consumer outside BuildCorrespondence: RansacCurvature::getFitness
 * (GlobalRegistration/RansacCurvature.h:661-704) for n_hyp pose hypotheses of ONE (source, target) pair in one
 * launch -- the RANSAC loop calls it once per hypothesis, up to max_iteration = 4 000 000 times per pair.
 * M: n_hyp row-major FLOAT 4x4 (final_transformation_ candidates).  inliers[h] = #{i : NN sqdist(M_h * src[i], tgt)
 * < corr_dist_threshold^2} (exact); fitness[h] (nullable) = mean of those squared distances (float64 sum; the
 * reference adds float32 in point order) or FLT_MAX when there is no inlier. */
int er_ransac_fitness_batch(er_cloud_t src, er_cloud_t tgt, int n_hyp, const float* M, float corr_dist_threshold,
                            int* inliers, double* fitness);

/* The accepted hypothesis, with the lists: getFitness's `inliers` / `inliers_target` (RansacCurvature.h:661-704) and
 * getInformation (:707-733) in one call.  pairs_host receives min(*n_inliers, capacity) (target index, source index)
 * pairs -- the layout of er_find_correspondence -- in ascending source index, the reference's push_back order;
 * *fitness (nullable) as above; info_source36 / info_target36 (nullable, row-major 6x6) = sum A^T A over the inlier
 * source points / their matched target points. */
int er_ransac_inliers(er_cloud_t src, er_cloud_t tgt, const float* M16, float corr_dist_threshold, int* pairs_host, int capacity,
                      int* n_inliers, double* fitness, double* info_source36, double* info_target36);

/* ---- GlobalRegistration: the RANSAC pose search (RansacCurvature::computeTransformation, RansacCurvature.h:411-657, with
 * PolyRejector.h), the per-point features as an input (setSourceFeatures / setTargetFeatures, GlobalRegistration.cpp:131-147). ---- */
typedef struct er_features_s* er_features_t;

/* n descriptors of dim floats (33 for FPFH; 1 <= dim <= 64), row i belongs to point i of a cloud in file order.  Values must be
 * finite and at most 1e15 in magnitude (squared distances then stay finite). */
int er_features_create(const float* feat_host, int n, int dim, int device, er_features_t* out);
int er_features_destroy(er_features_t f);
int er_features_size(er_features_t f);

/* findSimilarFeatures' nearestKSearch (RansacCurvature.h:373-387) for EVERY source descriptor at once: its k nearest target
 * descriptors by brute force, 1 <= k <= 8 and k <= n_tgt.  Distance = float32 sum of squared differences in ascending dimension; ascending
 * distance, ties to the lower target index.  idx_host / sqdist_host (either may be NULL): [n_src][k]. */
int er_feature_knn(er_features_t src, er_features_t tgt, int k, int* idx_host, float* sqdist_host);

/* The unit under the loop, for explicit samples: n_hyp hypotheses of nr_samples (3 .. 6) pairs (source point sample_idx[h][i], target
 * point corr_idx[h][i]).  Per hypothesis, in the reference's order (:524-613): thresholdPolygon over ALL pairs of edges (float32 squared
 * lengths, min/max ratio against similarity^2), the rigid estimate of the pairs (least squares, float64, rounded to float32 once),
 * NaN check, thresholdNormal (every n_t . (R n_s) >= cos(angle_diff), float32).  status[h]: 0 accepted, 1 polygon, 2 normal / NaN.
 * M: n_hyp row-major float 4x4 (all zero for status 1; the estimate for status 0 and 2). */
int er_ransac_hypotheses(er_cloud_t src, er_cloud_t tgt, int n_hyp, int nr_samples, const int* sample_idx, const int* corr_idx,
                         float similarity, float angle_diff, int* status, float* M);

typedef struct er_ransac_params {
  int max_iterations;        /* 4000000   (alignment.config)        1 .. 2^28 */
  int nr_samples;            /* 4         3 .. 6; 2 is refused: the reference's two-point branch builds the target's virtual points
                                          from the SOURCE's normal and midpoint (:575-580), matching it would mean copying a slip */
  int k_correspondences;     /* 2         1 .. 8 */
  float similarity;          /* 0.9       [0, 1) */
  float max_corr_dist;       /* 0.075     <= the target cloud's grid cell */
  float inlier_fraction;     /* 0.33      [0, 1] */
  int inlier_number;         /* 30000 */
  float angle_diff;          /* 0.52359878 */
  unsigned int seed;
  int chunk_iterations;      /* iterations per round of launches; 0 = 1048576.  NOT part of the result. */
} er_ransac_params;
typedef struct er_ransac_stats {   /* the reference's debug line (:655) */
  long long iterations, polygon_rejections, normal_rejections, scored;
} er_ransac_stats;
typedef struct er_ransac_aux {     /* one scored hypothesis (writeAuxData's list, :737-747, plus its score) */
  int iteration, count;
  double error;
  float M[16];
} er_ransac_aux;
int er_ransac_params_default(er_ransac_params* p);

/* computeTransformation with an identity guess, all on the device.  Iteration i draws its random numbers from (seed, i, draw) only:
 *   z = (seed << 32) + 16 i + draw;  z += 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31;  r = z >> 32;  index(m) = (m * r) >> 32        (64-bit unsigned)
 * draws 0 .. nr_samples-1 feed selectSamples (:319-359, index(n - i)), draw 8 + i picks index(k) among the k feature matches of the
 * i-th (ascending) sample when k > 1 (:383-386).  Survivors of the polygon test are estimated, normal-tested and scored like
 * er_ransac_fitness_batch (count exact; the sum of the inlier distances in 64-bit fixed point, so that error = sum / count is a
 * function of the inlier set alone).  Acceptable: (float)count / n_src >= inlier_fraction or count > inlier_number, and count > 0;
 * the acceptable hypothesis of lowest error wins, the earliest iteration on equal error (:627-643).
 * None acceptable: *converged = 0 and T_out = identity (the reference leaves final_transformation_ = guess).
 * aux (nullable): the first aux_capacity scored hypotheses in iteration order; *aux_count (nullable) = how many were scored.
 * The result -- T_out, n_inliers, error, stats, aux -- is a function of the clouds, the features and the parameters other than
 * chunk_iterations: not of the chunking, the grid sizes or the run. */
int er_ransac_align(er_cloud_t src, er_cloud_t tgt, er_features_t src_feat, er_features_t tgt_feat, const er_ransac_params* p,
                    float T_out[16], int* converged, int* n_inliers, double* error, er_ransac_stats* stats, er_ransac_aux* aux,
                    int aux_capacity, int* aux_count);

/* The pair loop of do_all (GlobalRegistration.cpp:38-41) in one call: n_pairs searches (src[i], tgt[i], src_feat[i], tgt_feat[i]) on ONE device
 * under one parameter set; a cloud may appear in any number of pairs, in either role.  seeds (nullable): one seed per pair instead of p->seed.
 * Outputs are arrays over the pairs -- T_out n*16 floats, converged n ints, n_inliers / error / stats (nullable) n entries -- and equal, bit for
 * bit, what er_ransac_align returns for each pair alone (with that pair's seed): every kernel of the search takes the pair from a grid axis, the
 * pairs share nothing but the launches.  info_source36 / info_target36 (nullable, n row-major 6x6 float64 matrices): getInformation
 * (RansacCurvature.h:706-733) at the winning transform, bit-equal to er_ransac_inliers called with it; all zero for a pair that did not converge.
 * The pairs run in waves of max_concurrent; a wave shares one workspace allocation, one stream and one read-back of its states.  A pair in flight
 * needs 88 bytes and one bit per chunk iteration (92 MB at the default chunk of 1048576) plus its k-NN table.  max_concurrent = 0: as many pairs as
 * fit into 2 GiB of that workspace, at least 1 and at most 64 (23 at the default chunk).  Neither max_concurrent nor the order or make-up of the
 * list is part of any pair's result.
 * Everything er_ransac_align refuses is refused for the whole list before the first launch, the message naming the pair ("pair 3: ..."); also
 * max_concurrent < 0, n_pairs < 0 and a NULL array for n_pairs > 0.  n_pairs == 0 returns 0 and touches nothing. */
int er_ransac_align_batch(int n_pairs, const er_cloud_t* src, const er_cloud_t* tgt, const er_features_t* src_feat, const er_features_t* tgt_feat,
                          const er_ransac_params* p, const unsigned int* seeds, int max_concurrent, float* T_out, int* converged, int* n_inliers,
                          double* error, er_ransac_stats* stats, double* info_source36, double* info_target36);

/* ---- GlobalRegistration: the first half of do_all (GlobalRegistration.cpp:59-128) -- voxel-grid downsampling, normal and FPFH
 * estimation -- once per fragment, from a cloud that is already on the device.  The PCL calls are pinned to the float64 restatement of
 * tests/fpfh_restatement.py (PCL itself is not vendored).  A radius neighbourhood of point i: every point j of the same cloud whose
 * float32 squared distance ((dx*dx) + dy*dy) + dz*dz is < fl32(r * r), i itself included.  Every result is a function of the cloud and
 * the parameters alone: the same bits from run to run.  All entry points return an error -- never fault -- for NULL handles, an empty
 * cloud and a leaf or radius that is not positive and finite; the two radius queries also refuse a cloud that spans more than 4000 cells
 * of that radius along one axis (beyond it the float32 cell coordinates no longer guarantee exact membership). ---- */

/* The cloud's rows back on the host, in file order (either pointer may be NULL): [n][3] floats each. */
int er_cloud_read(er_cloud_t c, float* xyz_host, float* normal_host);

/* pcl::VoxelGrid<PointNT> at leaf (:59-68; all fields averaged, min_points_per_voxel 0): inv = fl32(1 / leaf), ijk = floor(fl32(x * inv)),
 * key = (i - min_i) + (j - min_j) div_x + (k - min_k) div_x div_y; one output point per occupied key in ascending key order, each of
 * x, y, z, nx, ny, nz the mean of the cell's members (float64 sum in file order / count, rounded to float32 once; normals are not
 * renormalised).  *out is a new cloud with a search grid for grid_cell; *n_out (nullable) its size.  Refused: a grid of more than
 * INT_MAX cells, where PCL warns and returns the cloud unfiltered. */
int er_cloud_voxel_grid(er_cloud_t in, float leaf, float grid_cell, er_cloud_t* out, int* n_out);

/* pcl::NormalEstimation at radius followed by the flip of :93-116: per point the float64 centroid and scatter matrix of its
 * neighbourhood, the unit eigenvector of the smallest eigenvalue, negated if its float64 dot product with the point's input normal is
 * < 0, rounded to float32.  Fewer than 3 neighbours: NaN (PCL leaves what its solver returns for a rank-deficient matrix).  *out: the same
 * points with the new normals and the input's grid cell; the input is not changed.  n_neighbours_host (nullable): [n] neighbourhood sizes. */
int er_cloud_estimate_normals(er_cloud_t in, float radius, er_cloud_t* out, int* n_neighbours_host);

/* pcl::FPFHEstimation at radius (:121-128) over the cloud's own points and normals, pair features and sums in float64.
 * SPFH of point i: integer counts [3][11] of the bins of (f1, f2, f3) = computePairFeatures(i, j) over its neighbours j != i, failed pairs
 * skipped; m_i = neighbours - 1; row = count * 100 / m_i.  FPFH of i: per bin the sum over neighbours j with d^2 != 0 of
 * spfh_j[bin] * (1 / d^2), every block of 11 scaled to sum 100, rounded to float32; a zero row for a point whose own normal is not finite.
 * *out: 33-dimensional features, row i for point i.  spfh_counts_host (nullable): int [n][33]; n_neighbours_host (nullable): int [n],
 * the point itself included. */
int er_fpfh_estimate(er_cloud_t c, float radius, er_features_t* out, int* spfh_counts_host, int* n_neighbours_host);

/* The descriptors back on the host: [n][er_features_dim] floats. */
int er_features_dim(er_features_t f);
int er_features_read(er_features_t f, float* feat_host);

/* Frees the pooled ICP workspaces (streams, scratch, pinned blocks).  Optional; call when no ICP call is running. */
int er_icp_release_workspaces(void);

/* CCorresApp::Registration (CorresApp.cpp:212-319) followed by CCorresApp::FindCorrespondence (:112-210) for a whole pair list in ONE call:
 *   counts[i]    the pre-check count of :257-264 (NN of T_guess * source within reg_dist);
 *   accepted[i]  the accept rule of :270 -- counts >= reg_num, or both ratios counts / |target| and counts / |source| above reg_ratio;
 *   T_final      16 floats per pair: icp.align from the float32 cast of the guess (:295-312) for an accepted pair, the cast of the guess itself
 *                for a rejected one (its transformation_ is left alone, :277-283); iterations / converged (nullable) as er_icp_align_batch;
 *   pairs_host, capacity, n_pairs, info36 (nullable): FindCorrespondence of the accepted pairs at the float64 cast of T_final (:312), as
 *                er_find_correspondence_batch returns them; n_pairs = 0 for a rejected pair.  The `Reduced too much` rule of :164-173
 *                (n_pairs / counts < 0.5) is the caller's: both numbers are returned.
 * The list is cut into ER_ICP_SHARES (default 6, at least ~8 pairs each) contiguous shares that run their three stages on a host thread and workspace each, so one
 * share's host round trips and PCIe list copies overlap the kernels of the others; the results are those of the three *_batch calls, bit for bit. */
int er_registration_batch(int n, const er_cloud_t* src, const er_cloud_t* tgt, const double* T_guess, double reg_dist, int reg_num, double reg_ratio,
                          int max_iter, double transformation_epsilon, int stop_rule, double corr_dist, double normal_cos, int* counts,
                          int* accepted, float* T_final, int* iterations, int* converged, int* const* pairs_host, const int* capacity,
                          int* n_pairs, double* info36);

/* ------------------------------------------------ depth odometry ---- */
/* The step that produces the pipeline's trajectory in the first place: KinFu-style projective point-to-plane ICP between depth frames,
 * batched over a pair list.  The reference tree does not contain KinFu (it lives in the author's PCL fork): every entry below restates
 * tests/odometry_restatement.py, the numpy statement of DESIGN.md 7.11, and NOTHING here is checked against PCL.
 * Per frame: 13x13 bilateral filter (sigma_space 4.5 px, sigma_depth 30 mm, weights from two host-built float32 tables), a pyramid of
 * 5x5 integer means of the taps within 3 sigma_depth of the centre, and per level a map of {vertex, normal} records (float32).  Per pair
 * and iteration: project every pixel of the current frame into the model frame, test distance and normal angle, 27 float64 sums of exact
 * products + a count, added in an order that depends on (cols, rows, level) only; a 6x6 float64 Cholesky solve and the pose update stay on
 * the device.  A pair's result is the same bits alone, in any list, in any order, for any window, on any run. */
typedef struct er_odom_s* er_odom_t;
typedef struct er_odom_params {
  int levels;             /* pyramid levels, 1 .. 4 (3) */
  int iterations[4];      /* iterations at level 0 (finest) .. 3: (10, 5, 4, 4); the loop runs from level levels-1 down to 0 */
  int bilateral;          /* 1; 0 copies the frame */
  int max_depth_mm;       /* depths above it are zeroed in level 0 before anything is derived from it; 0 = off (0) */
  int min_valid;          /* a pair with fewer matched pixels in an iteration is lost (50) */
  float dist_thresh;      /* reject a match farther than this, metres (0.10) */
  float angle_thresh;     /* reject a match whose |cross(ng, nm)| is >= this sine (sin 20 deg) */
} er_odom_params;
int er_odom_params_default(er_odom_params* p);

/* Restates odometry_restatement.Odometry(cols, rows, cam, params): frames of cols x rows uint16 millimetres, cam4 = (fx, fy, cx, cy) of
 * level 0 (level l uses cam4 / 2^l).  cols and rows must be divisible by 2^(levels-1).  Not thread-safe: one call per handle at a time. */
int er_odom_create(int cols, int rows, const float* cam4, const er_odom_params* params, int device, er_odom_t* out);
int er_odom_destroy(er_odom_t h);

#define ER_ODOM_OK 0
#define ER_ODOM_LOST 1
#define ER_ODOM_TRACE 17   /* doubles per traced iteration: the row-major 4x4 pose after it, then its matched-pixel count */
/* Restates odometry_restatement.Odometry.align for every pair of a list: pair p aligns current frame frame_idx[p] to model frame
 * model_idx[p] of depth[n_frames][rows * cols] (host memory, or device memory of the handle's device when depth_on_device), starting from
 * guess[p][16] (row-major float64 m_T_c; NULL = identity).  T_out[p][16]: m_T_c, float64 row-major.  status[p]: ER_ODOM_OK or ER_ODOM_LOST
 * (an iteration matched fewer than min_valid pixels, a Cholesky pivot was not positive, or something was not finite: the pair keeps its
 * last good pose).  trace (nullable): [n_pairs][sum of iterations over the levels used][ER_ODOM_TRACE], coarse to fine; sums (nullable):
 * [n_pairs][27], the last iteration's 21 entries of the upper triangle of J^T J row by row, then J^T r (rows (cross(vg, nm), nm)).
 * window: frames resident at a time (>= 2; 0 = what keeps the frame slab under 2 GiB).  The list is cut into runs of pairs whose frames fit
 * the window; a frame that the next run needs again stays resident. */
int er_odom_align_pairs(er_odom_t h, int n_frames, const uint16_t* depth, int depth_on_device, int n_pairs, const int* model_idx,
                        const int* frame_idx, const double* guess, double* T_out, int* status, double* trace, double* sums, int window);

/* Restates odometry_restatement.Odometry.track: er_odom_align_pairs of the list (i, i + 1), i = 0 .. n_frames - 2, from the identity.
 * T_rel[i][16] = frame i <- frame i + 1. */
int er_odom_track(er_odom_t h, int n_frames, const uint16_t* depth, int depth_on_device, double* T_rel, int* status, int window);

/* Frame-to-model alignment: every frame of depth[n_frames][rows * cols] against ONE model, whose side of the pair is not a
 * depth frame but the record maps of er_tsdf_raycast -- model_rec_dev[l], l = 0 .. levels - 1 (an array in host memory of pointers to device
 * memory of the handle's device): level l ray-cast at cols / 2^l x rows / 2^l with cam4 / 2^l, the intrinsics the handle uses for that
 * level.  The maps are copied device to device into a slot that is never preprocessed and stays resident over the runs of the list;
 * everything after that is er_odom_align_pairs' loop, unchanged, and the other arguments are its: guess[i][16] (NULL = identity), T_out[i][16]
 * = m_T_c of frame i (model <- frame), status, trace, sums, window.  Restates raycast_restatement.align_model.  A frame's result is the same
 * bits alone and in any list.  (Named apart from the er_odom_ family, whose list the odometry's own tests pin.) */
int er_frame_to_model_align(er_odom_t h, const void* const* model_rec_dev /* [levels], device */, int n_frames, const uint16_t* depth,
                            int depth_on_device, const double* guess, double* T_out, int* status, double* trace, double* sums, int window);

/* The same against n_models models, one per frame: frame i is aligned against model model_of_frame[i]; model k's record maps are
 * model_rec_dev[k * levels + l].  er_frame_to_model_align is the n_models == 1 case, bit for bit, and a frame's result is what that call gives
 * for the frame and its model alone -- in any list, in any order, for any window. */
int er_frames_to_models_align(er_odom_t h, int n_models, const void* const* model_rec_dev /* [n_models][levels], device */, int n_frames,
                              const uint16_t* depth, int depth_on_device, const int* model_of_frame /* [n_frames] */, const double* guess,
                              double* T_out, int* status, double* trace, double* sums, int window);

/* Restates odometry_restatement.Odometry.linearize: ONE evaluation of the 27 sums and the count at the pose T (m_T_c) on `level`, for
 * depth2 = {model frame, current frame}. */
int er_odom_linearize(er_odom_t h, const uint16_t* depth2, int on_device, int level, const double* T, double* sums, int* count);

/* Restates odometry_restatement.Odometry.maps for one frame (any output may be NULL): depth_out uint16 [rows_l * cols_l] (level 0: the
 * filtered, depth-limited frame), vmap_out / nmap_out float [rows_l * cols_l][3], NaN where invalid. */
int er_odom_read_maps(er_odom_t h, const uint16_t* depth1, int on_device, int level, uint16_t* depth_out, float* vmap_out, float* nmap_out);

/* Restates odometry_restatement.tables(): the two weight tables of the bilateral filter as the kernels read them.  space[dx^2 + dy^2],
 * 73 entries; depth_w[|delta| in mm], *n_depth_w entries (at most ER_ODOM_DEPTH_W), zero beyond.  Works without a device. */
#define ER_ODOM_DEPTH_W 512
int er_odom_tables(float* space, float* depth_w, int* n_depth_w);

/* ------------------------------------------------ fragments from a depth stream ---- */
/* The step that comes before everything else in the pipeline (pcl_kinfu_largeScale in the author's PCL fork; not in the reference tree):
 * a depth stream is cut into fragments of `interval` frames, every fragment is tracked frame-to-model against a TSDF volume of its own and
 * leaves its frame poses and the oriented surface points of that volume (cloud_bin_<k>.pcd).  `lanes` fragments run in lockstep: one ray-cast
 * launch, one alignment run and one integration per lane and step.
 * THE CONTRACT: fragment k's poses and statuses are the bits of DepthOdometry.track_model (odometry.py) on its frames with its T0 on a fresh
 * volume, its points and normals the bits of TSDFVolume.SaveFragment of that volume -- for any lanes, host or device depth, any run. */
typedef struct er_frag_s* er_frag_t;
typedef struct er_frag_params {
  int interval;               /* frames per fragment (50) */
  int lanes;                  /* fragments in flight, 1 .. 64 (8); NOT part of any result */
  int max_units;              /* unit pool of each lane's volume (512) */
  float length;               /* edge of the fragment cube, metres (3.0) */
  er_raycast_params raycast;  /* the model's ray-cast (er_raycast_params_default) */
} er_frag_params;
int er_frag_params_default(er_frag_params* p);
/* cam6 as er_tsdf_create (NULL = its defaults); odom_params / frag_params NULL = the defaults.  Every lane owns an er_tsdf_t of max_units units:
 * at 640 x 480 roughly 0.85 GB of batch staging plus max_units x 2 MiB.  A lane that cannot be allocated is a refusal that names the bytes. */
int er_frag_create(int cols, int rows, const float cam6[6], const er_odom_params* odom_params, const er_frag_params* frag_params, int device,
                   er_frag_t* out);
int er_frag_destroy(er_frag_t h);
int er_frag_lane_bytes(er_frag_t h, size_t* bytes);   /* device memory the first lane took at create (measured) */
/* Fragment k = frames [k interval, min((k + 1) interval, n_frames)); a short last fragment is a fragment.  depth: n_frames * rows * cols uint16
 * millimetres, host memory (uploaded once) or complete device memory.  T0: the pose of every fragment's first frame -- n_T0 == 1: one for all,
 * n_T0 == the fragment count: one each, NULL: the kinfu convention, (length / 2, length / 2, -0.3) looking along +z.  Frame i of a fragment:
 * the volume is ray-cast at W_{i-1}, the frame aligned against it from the identity, W_i = W_{i-1} m_T_c, the frame integrated at W_i; a lost
 * frame keeps W_{i-1} and is not integrated.  W_out[n_frames][16], status[n_frames] (ER_ODOM_OK / ER_ODOM_LOST; a fragment's first frame is
 * never lost).  The fragments' points stay with the handle until the next call: er_frag_count, er_frag_read. */
int er_frag_build(er_frag_t h, int n_frames, const uint16_t* depth, int depth_on_device, const double* T0, int n_T0, double* W_out, int* status);
int er_frag_count(er_frag_t h, int* n_fragments);
/* xyz_out / normals_out: [count][3] floats, the points inside 0 <= x, y, z < length, NaN-normal rows kept.  Both NULL: only the count. */
int er_frag_read(er_frag_t h, int fragment, float* xyz_out, float* normals_out, long capacity, long* count);

/* ------------------------------------------------ pose graph optimisation ---- */
/* GraphOptimizer: the candidate loop closures of GlobalRegistration in, pruned closures and fragment poses out.  The model is the
 * reference's (GraphOptimizer/OptApp.cpp over g2o's VertexSE3 / EdgeSE3 and vertigo's switchable edge); g2o itself cannot be built from
 * the reference tree, so every entry below restates tests/posegraph_restatement.py, the numpy statement of DESIGN.md 7.12, and NOTHING
 * here is checked against g2o.  The Levenberg-Marquardt schedule is this project's.  float64 throughout; poses are
 * row-major 4x4; every switch is eliminated inside its edge, so the system that is factored is dense 6 (n_poses - 1) square.  The loop
 * stays on the device: per trial the host reads one small record.  A graph gives the same bits on every run. */
typedef struct er_pgo_s* er_pgo_t;
#define ER_PGO_SWITCHABLE 0   /* COptApp::OptimizeSwitchable (OptApp.cpp:51-159) */
#define ER_PGO_EM 1           /* COptApp::OptimizeEM (OptApp.cpp:161-265) */

/* COptApp::Init (OptApp.cpp:28-49) and the graph both modes build (OptApp.cpp:76-128, 185-225): n_poses vertices (2 .. 1024), vertex 0
 * fixed, initial poses X_{i+1} = X_i odo_T[i]; odometry edge i joins i and i + 1 (odo_T[n_poses - 1][16], odo_info[n_poses - 1][36] or NULL
 * for the identity); loop edge k joins loop_ids[2k] and loop_ids[2k + 1] (loop_T[n_loops][16], loop_info[n_loops][36] or NULL).  Several
 * loop edges on one pair and id1 > id2 are allowed.  Refused, naming the entry: id1 == id2, an id out of range, a non-finite entry. */
int er_pgo_create(int n_poses, int n_loops, const double* odo_T, const double* odo_info, const int* loop_ids, const double* loop_T,
                  const double* loop_info, int device, er_pgo_t* out);
int er_pgo_destroy(er_pgo_t h);

/* optimizer->optimize(max_iteration) of OptimizeSwitchable, or the max_iteration E / M rounds of OptimizeEM (OptApp.cpp:130-131, 227-249),
 * from the initial poses and all switches at 1, whatever an earlier call left.  weight: --weight (the switch prior's information, or the
 * EM scale).  poses_out[n_poses][16]; switch_or_weight_out[n_loops]: the switches s_k (an edge is kept when s_k > 0.5) or the last E
 * step's l_k (kept when l_k > 0.25).  *iterations, *trials (nullable): LM iterations begun and trials made.  chi2_trace (nullable):
 * [10 * max_iteration][4] = (lambda of the trial, F before it, F of the candidate, accepted), one row per trial. */
int er_pgo_optimize(er_pgo_t h, int method, double weight, int max_iteration, double* poses_out, double* switch_or_weight_out, int* iterations,
                    int* trials, double* chi2_trace);

/* Measurement (scripts/posegraph_probe.py): with profiling on, HIP events round the stages of every trial; er_pgo_get_profile returns the
 * milliseconds of the last er_pgo_optimize summed over its trials: linearise, assemble, factor, solve, apply + evaluate. */
int er_pgo_set_profiling(er_pgo_t h, int on);
int er_pgo_get_profile(er_pgo_t h, double* stage_ms5);

/* Test hooks.  The current state: poses[n_poses][16], switches[n_loops] (either may be NULL). */
int er_pgo_set_state(er_pgo_t h, const double* poses, const double* switches);
int er_pgo_get_state(er_pgo_t h, double* poses, double* switches);
/* Restates posegraph_restatement.Graph.linearize (switchable mode) at the current state: the reduced dense system H_out[n][n] (full
 * symmetric, lambda only inside every switch's H_ss), b_out[n], n = 6 (n_poses - 1), and chi2_out[n_poses - 1 + n_loops] = r^T Omega r of
 * every edge, odometry first. */
int er_pgo_linearize(er_pgo_t h, double weight, double lambda, double* H_out, double* b_out, double* chi2_out);
/* Restates posegraph_restatement.Graph.trial: ONE factor of H + lambda I, solve and apply, without deciding; the current state stays.
 * dx_out[n], ds_out[n_loops] (before the clamp), *F_new_out = F of the candidate, *status_out = 1 when a pivot was not positive and finite. */
int er_pgo_trial(er_pgo_t h, double weight, double lambda, double* dx_out, double* ds_out, double* F_new_out, int* status_out);

/* ------------------------------------------ next consumer: FragmentOptimizer ---- */
typedef struct er_fopt_s* er_fopt_t;

/* COptApp's point clouds (FragmentOptimizer/OptApp.cpp:74-98, PointCloud.h): num fragments over a control lattice of
 * (resolution+1)^3 vertices, cube edge `length`. */
int er_fopt_create(int num, int resolution, float length, int device, er_fopt_t* out);
int er_fopt_destroy(er_fopt_t h);

/* PointCloud::LoadFromXYZNFile / LoadFromPCDFile body (PointCloud.cpp:22-63): n points (xyz, normals; NaN-normal points
 * already dropped) through GetCoordinate (PointCloud.h:92-176).  Like the reference, loading stops at the first point
 * outside the cube; *first_out_of_bound (nullable) receives its index or -1.  Replacing a cloud drops the correspondence lists. */
int er_fopt_set_cloud(er_fopt_t h, int frag, const float* xyz_host, const float* normal_host, int n, int* first_out_of_bound);
int er_fopt_cloud_size(er_fopt_t h, int frag);
/* Point state read-back (any pointer may be NULL): idx_[0], val_[8], nval_[8], p_[3], n_[3] per point. */
int er_fopt_get_points(er_fopt_t h, int frag, int* idx0, float* val, float* nval, float* p, float* n);

/* PointCloud::UpdatePose (PointCloud.h:71-83): p_, n_ <- M * (p_,1), M * (n_,0); M row-major FLOAT 4x4. */
int er_fopt_update_pose(er_fopt_t h, int frag, const float M[16]);
/* PointCloud::UpdateAllPointPN (PointCloud.h:44-52): p_, n_ from the fragment's slice of expand_ctr (nper doubles). */
int er_fopt_update_point_pn(er_fopt_t h, int frag, const double* ctr_slice_host);

/* COptApp::InitCorrespondences (OptApp.cpp:100-118): n_pairs lists of (index in fragment frag_i, index in frag_j) rows =
 * the lines of corres_<i>_<j>.txt.  Sorted once by lattice cell pair for the assembly kernels. */
int er_fopt_set_correspondences(er_fopt_t h, int n_pairs, const int* frag_i, const int* frag_j, const int* const* pairs_host,
                                const int* counts);
/* The same with the lists ALREADY IN HBM on the handle's device (pairs_dev[l] = device pointer to counts[l] rows, e.g. the buffers
 * er_registration_batch filled): the (cell, cell) keys, ONE stable radix sort over all lists, the run lengths and the gather run on the
 * GPU; only the group table (a few thousand rows) visits the host.  Same order as the host path -- lists in the given order, groups by
 * ascending cell pair, rows of a group in list order -- hence bit-identical assembly results.  Row indices are range-checked on the device. */
int er_fopt_set_correspondences_dev(er_fopt_t h, int n_pairs, const int* frag_i, const int* frag_j, const int* const* pairs_dev,
                                    const int* counts);
int er_fopt_group_count(er_fopt_t h);          /* groups = distinct (pair, lattice cell of p_i, lattice cell of p_j) */
int er_fopt_group_info(er_fopt_t h, int* info4);   /* 4 ints per group: frag_i, frag_j, idx_[0] of p_i's cell, of p_j's cell */
/* PointCloud::UpdateAllNormal (PointCloud.h:32-36): n_ only, from the fragment's slice of ctr (non-rigid mode, OptApp.cpp:151-153). */
int er_fopt_update_normals(er_fopt_t h, int frag, const double* ctr_slice_host);

/* Hessian assembly of OptimizeRigid (OptApp.cpp:312-375): JJ = (6 num)^2 row-major FULL symmetric matrix including the
 * "+1" every pair puts on the first six diagonal entries, Jb (6 num), score = sum b^2.  Host output buffers. */
int er_fopt_assemble_rigid(er_fopt_t h, double* JJ, double* Jb, double* score);
/* Data term of OptimizeSLAC (OptApp.cpp:473-560): JJ = (6 num + nper)^2 row-major, UPPER triangle as the reference
 * accumulates it (before baseJJ and the gauge "+1"s), Jb, score.  pose_rot_t: num * 9 doubles, row-major
 * pose_[l].block<3,3>(0,0).transpose(). */
int er_fopt_assemble_slac(er_fopt_t h, const double* pose_rot_t, double* JJ, double* Jb, double* score);

/* Data term of OptimizeNonrigid (OptApp.cpp:159-206), block-sparse as it is born:
 *   diag    [num][(resolution+1)^3][24][24]  sum of mati / matj blocks per fragment and lattice cell (cell = its corner vertex
 *           idx_[0]/3); local index c*8 + t  <->  lattice index idx_[t] + c (t = vertex 4dx+2dy+dz, c = x,y,z); both triangles
 *   offdiag [groups][24][24]                 matij block of each group (rows: fragment i's cell, columns: fragment j's cell)
 * thisAA - baseAA is the sum of these blocks at their global positions (fragment * nper + lattice index); the host merges
 * blocks that share lattice vertices when it builds the sparse matrix for the solver. */
int er_fopt_assemble_nonrigid(er_fopt_t h, double weight, double* diag, double* offdiag);

/* The systems can stay where they are assembled and be solved there: Cholesky in HBM (the library's own recursive blocked
 * factorisation over rocBLAS level-3 calls, rocBLAS loaded on first use; dense, or block-sparse over fragments beyond ER_FOPT_DENSE_MAX
 * unknowns) instead of the reference's sparse CHOLMOD factorisation on the host.  A system that is not positive definite is an error
 * whose text names the 1-based index of the first non-positive pivot (CHOLMOD's status, OptApp.cpp:209-211, 389-393).  288 GB hold the non-rigid mode's dense
 * system up to ~180 k unknowns (82 fragments at resolution 8).
 *   er_fopt_factor_slac      thisJJ of one OptimizeSLAC iteration: data term + default_weight * (lattice Laplacian + anchor) +
 *                            the gauge "+1"s (OptApp.cpp:449-560, 811-846), factored.  dataJb_host (nullable, 6 num + nper) and
 *                            score (nullable) return the data term's right-hand side and error.
 *   er_fopt_factor_nonrigid  thisAA of one OptimizeNonrigid iteration: baseAA + data term (OptApp.cpp:155-211, 765-810), factored.
 *   er_fopt_solve            x = A^-1 rhs with the factor kept on the device (rhs + the device's dataJb when add_data_jb != 0). */
int er_fopt_factor_slac(er_fopt_t h, const double* pose_rot_t, double default_weight, double* dataJb_host, double* score);
int er_fopt_factor_nonrigid(er_fopt_t h, double weight);
int er_fopt_solve(er_fopt_t h, const double* rhs_host, int add_data_jb, double* x_host);
/* Test hook for the failure path of the factorisation: every system factored from now on gets `value` added to diagonal entry
 * `index` (0-based) after assembly and before the Cholesky; index < 0 switches it off.  Not used by any host program. */
int er_fopt_debug_shift_diagonal(er_fopt_t h, long index, double value);

#ifdef __cplusplus
}
#endif
#endif /* ER_HIP_H_ */
