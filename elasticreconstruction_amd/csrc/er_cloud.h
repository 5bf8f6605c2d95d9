// er_cloud.h -- what the translation units of path B (er_cloud.hip, er_icp.hip, er_ransac.hip, er_fpfh.hip) know about each other: the two handle types
// and the few functions one of them calls in another.  Internal: not part of the C ABI (include/er_hip.h).
#pragma once

#include "er_common.h"
#include "er_grid.h"
#include "er_mem.h"

#include "../../include/er_hip.h"

#include <algorithm>
#include <vector>

namespace er {
struct CloudSlab;   // one device allocation shared by the clouds of a chunk (er_cloud.hip)
}

struct er_cloud_s {
  int device = 0, n = 0;
  float *xyz = nullptr, *nrm = nullptr;
  float4* sorted = nullptr;
  float4* xn = nullptr;         // [2n] file order: {x, y, z, 0}, {nx, ny, nz, 0} -- ONE 32-byte gather per matched point in k_icp_iter
  int* cell_start = nullptr;
  er::Grid grid{};
  float radius_cap = 0.f;       // largest search radius the grid supports
  float nmax = 1.f;             // largest finite |normal component| (k_chunk_bounds): bounds the ICP sums (PairDev::fx_scale)
  er::CloudSlab *pts_slab = nullptr, *cell_slab = nullptr;   // the chunk's allocations these pointers live in
};

struct er_features_s {
  int device = 0, n = 0, dim = 0, dp = 0;     // dp = dim rounded up to a multiple of 8 (rows padded with zeros: they add +0 to a distance)
  er::Buffer<float> d;                        // [n][dp]
};

namespace er {

inline int nblocks_of(int n) { return (std::max(n, 1) + kBlock - 1) / kBlock; }

// ---- er_cloud.hip ----
// (er::cloud_create_device, the cloud builder for rows that already live on the device, is declared in er_common.h: er_tsdf_extract.hip calls it too.)

int no_device(const char* who);
int check_pair(er_cloud_t src, er_cloud_t tgt, double radius, const char* who);

// The bounding box of a cloud from its rows in device memory: k_chunk_bounds of the grid builder on `stream`, which is synchronised.
int cloud_bounds(const er_cloud_s* c, hipStream_t stream, float lo[3], float hi[3]);

// hipcub's DeviceRadixSort::SortPairs<unsigned, unsigned> and DeviceScan::InclusiveSum<int*, int*>, arguments in hipcub's order and with hipcub's
// convention (tmp == nullptr: only tmp_bytes is set): the one translation unit that includes hipcub instantiates them once.
hipError_t sort_pairs_u32(void* tmp, size_t& tmp_bytes, const unsigned* keys_in, unsigned* keys_out, const unsigned* values_in, unsigned* values_out,
                          int n, int begin_bit, int end_bit, hipStream_t stream);
hipError_t inclusive_sum_i32(void* tmp, size_t& tmp_bytes, int* in, int* out, int n, hipStream_t stream);

// ---- er_icp.hip ----
// The compute stream of a group workspace borrowed from the per-device pool that er_icp_release_workspaces empties; the destructor drains the
// workspace's streams and returns it.
struct StreamLease {
  hipStream_t stream = nullptr;
  StreamLease() = default;
  StreamLease(const StreamLease&) = delete;
  StreamLease& operator=(const StreamLease&) = delete;
  ~StreamLease();
  int acquire(int device);
  // getInformation for m pairs at one float 4x4 each (er_ransac_inliers without its lists), through the leased workspace's compaction chain on
  // `stream`; waits for the result.  info_source36 / info_target36 (either may be NULL): m row-major 6x6 matrices.
  int ransac_information(int m, const er_cloud_t* src, const er_cloud_t* tgt, const float* M16, float corr_dist_threshold, double* info_source36,
                         double* info_target36);

 private:
  void* group_ = nullptr;
};

}  // namespace er
